/* moshi_mi.h — C ABI of libmoshi_mi.so: the MI355X-native (gfx950) engine for the 12.5 Hz
 * full-duplex frame step of kyutai-labs/moshi:
 *
 *      MimiModel.encode  ->  LMGen.step  ->  MimiModel.decode
 *
 * Each entry point replaces one method of the reference's PyTorch model API (the reference has
 * no FFI of its own for this path; its boundary is the Python surface of
 * moshi/moshi/models/compression.py and moshi/moshi/models/lm.py).  The citation on every
 * function is the reference method it stands in for (path:line under the reference checkout).
 *
 * Conventions
 *   - Plain C, no torch types.  All tensor pointers are DEVICE pointers on the current HIP device
 *     unless the comment says "host".  The caller owns every I/O buffer; a handle owns its packed
 *     weights and all streaming state (conv histories, conv-transpose partials, ring KV caches,
 *     delay token ring, offsets, exec masks).
 *   - Every function returns 0 (MMI_OK) or a negative mmi_status; nothing throws across the ABI.
 *     mmi_last_error() gives a thread-local human readable message for the last failure.
 *   - `stream` is a hipStream_t passed as void*.  Work is enqueued on it; nothing synchronises
 *     the device (same contract as the reference: "no hidden syncs in step", sampling.py:32-46).
 *   - One handle = one GPU = one caller at a time (not re-entrant), like a reference model
 *     instance (server.py:45,57 serialises sessions with a lock).  Independent handles on
 *     different GPUs may be driven from different processes (one process per GPU).
 *   - Integer tensors at the boundary are int64, as in the reference API.
 */
#ifndef MOSHI_MI_H_
#define MOSHI_MI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMI_ABI_VERSION 3

typedef enum mmi_status {
    MMI_OK = 0,
    MMI_ERR_INVALID = -1,        /* bad argument (null pointer, negative size...)                       */
    MMI_ERR_SHAPE = -2,          /* batch/shape mismatch: reference raises AssertionError (lm.py:679-686) */
    MMI_ERR_STATE = -3,          /* not streaming: reference raises RuntimeError (lm.py:673-676)          */
    MMI_ERR_HIP = -4,            /* a HIP runtime call failed                                           */
    MMI_ERR_MISSING_WEIGHT = -5, /* a state-dict key required by the config was not supplied             */
    MMI_ERR_UNSUPPORTED = -6,    /* config outside what the kernels implement                           */
    MMI_ERR_BUSY = -7,           /* batcher: no free slot / a channel's buffer is full                    */
    MMI_ERR_NO_CHANNEL = -8      /* batcher: the channel id names no open channel (closed, or re-opened under a new id) */
} mmi_status;

typedef enum mmi_dtype { MMI_F32 = 0, MMI_BF16 = 1, MMI_I64 = 2, MMI_F16 = 3, MMI_I8 = 4, MMI_F8E4M3 = 5 /* OCP e4m3fn */,
                         MMI_F4E2M1X2 = 6 /* OCP MXFP4 codes, two E2M1 per byte (element 2i in the low nibble) */,
                         MMI_E8M0 = 7 /* OCP MX block scale, 2^(s - 127) */ } mmi_dtype;

typedef void* mmi_stream; /* hipStream_t */

/* One state-dict entry, named exactly as in the reference checkpoints
 * (loaders.py:356-358,413-422).  `data` is a device pointer. */
typedef struct mmi_tensor_desc {
    const char* name;
    const void* data;
    int32_t dtype; /* mmi_dtype */
    int32_t ndim;
    int64_t shape[4];
} mmi_tensor_desc;

int mmi_version(void);
const char* mmi_last_error(void);

/* ------------------------------------------------------------------------------------------ */
/* Mimi codec                                                                                 */
/* ------------------------------------------------------------------------------------------ */

/* Mirrors loaders._seanet_kwargs / _quantizer_kwargs / _transformer_kwargs / _mimi_config
 * (loaders.py:38-88).  Fixed by the kernels: causal, pad_mode "constant", true_skip, ELU(1.0),
 * norm "none", n_residual_layers == 1 (dilation 1), transformer norm "layer_norm", gating "none",
 * positional_embedding "rope", learnt conv resampling with the channel-wise upsample. */
typedef struct mmi_mimi_cfg {
    int32_t sample_rate;      /* 24000 */
    int32_t frame_size;       /* samples per 12.5 Hz frame = 1920 (compression.py:244-246) */
    int32_t channels;         /* 1 */
    int32_t dimension;        /* 512 */
    int32_t n_filters;        /* 64 */
    int32_t n_ratios;         /* 4 */
    int32_t ratios[8];        /* decoder order {8,6,5,4}; the encoder uses them reversed (seanet.py:154) */
    int32_t kernel_size;      /* 7 */
    int32_t last_kernel_size; /* 3 */
    int32_t residual_kernel_size; /* 3 */
    int32_t compress;         /* 2 */
    int32_t resample_stride;  /* encoder_frame_rate / frame_rate = 2 (compression.py:197-207) */
    int32_t tr_d_model;       /* 512 */
    int32_t tr_num_heads;     /* 8 */
    int32_t tr_num_layers;    /* 8 */
    int32_t tr_dim_feedforward; /* 2048 */
    int32_t tr_context;       /* 250 */
    float tr_max_period;      /* 10000 */
    int32_t q_dimension;      /* 256 */
    int32_t q_bins;           /* 2048 */
    int32_t q_n_q;            /* 32 total codebooks */
    int32_t q_n_q_semantic;   /* 1 */
} mmi_mimi_cfg;

typedef struct mmi_mimi mmi_mimi;

/* loaders.get_mimi (loaders.py:323-363): build the model from state-dict tensors (fp32).
 * Weights are repacked into MFMA fragment order on the device; the descs may be freed after. */
int mmi_mimi_create(const mmi_mimi_cfg* cfg, const mmi_tensor_desc* weights, int32_t n_weights,
                    int32_t max_batch, mmi_mimi** out);
void mmi_mimi_destroy(mmi_mimi* m);

/* MimiModel.set_num_codebooks (compression.py:258-260). 1 <= n <= q_n_q. */
int mmi_mimi_set_num_codebooks(mmi_mimi* m, int32_t n);
int mmi_mimi_num_codebooks(const mmi_mimi* m);

/* StreamingModule.streaming(batch) enter / exit (streaming.py:131-137, 110-129): allocate and
 * zero the streaming state of `batch` rows; exec mask all ones. */
int mmi_mimi_streaming_start(mmi_mimi* m, int32_t batch, mmi_stream stream);
int mmi_mimi_streaming_stop(mmi_mimi* m);
/* Rows of the current stream (StreamingModule._streaming_state.batch_size); 0 when not streaming. */
int mmi_mimi_streaming_batch(const mmi_mimi* m);

/* StreamingModule.set_exec_mask (streaming.py:183-211): mask = device uint8[batch]. */
int mmi_mimi_set_exec_mask(mmi_mimi* m, const uint8_t* mask, mmi_stream stream);
/* StreamingModule.reset_streaming (streaming.py:139-156): mask = device uint8[batch] or NULL (= all rows). */
int mmi_mimi_reset(mmi_mimi* m, const uint8_t* mask_or_null, mmi_stream stream);

/* StreamingModule.get_streaming_state / set_streaming_state (streaming.py:158-181): the complete streaming state of the
 * current stream as one opaque device buffer of mmi_mimi_state_bytes() bytes (conv histories, conv-transpose partials, KV
 * rings, offsets, masks).  A snapshot can be loaded back into the same handle while it streams with the same batch. */
int64_t mmi_mimi_state_bytes(const mmi_mimi* m);
int mmi_mimi_state_save(mmi_mimi* m, void* dst, int64_t bytes, mmi_stream stream);
int mmi_mimi_state_load(mmi_mimi* m, const void* src, int64_t bytes, mmi_stream stream);
/* Fork session `src` into the sessions dst[0 .. n_dst) of the same stream (dst: a host array).  No reference counterpart: the
 * nearest is get_streaming_state / set_streaming_state on a batch of one (streaming.py:158-181); a whole-handle snapshot cannot
 * place one session's state into another slot.  Stream-ordered (no host synchronisation): after the call each destination is the
 * session `src` is - conv histories, conv-transpose partials, both transformer offsets and the valid rows of both KV rings,
 * the replicate-padding flag - its previous state is gone as after mmi_mimi_reset, and its exec bit is 1.  MMI_ERR_STATE when
 * not streaming; MMI_ERR_INVALID for src or a dst outside [0, batch), dst == src, a repeated dst, n_dst outside [1, 16]; a
 * refused call changes nothing. */
int mmi_mimi_fork_session(mmi_mimi* m, int32_t src, const int32_t* dst, int32_t n_dst, mmi_stream stream);

/* MimiModel.encode in streaming mode (compression.py:376-388, 338-374):
 * pcm f32 [batch,1,n_frames*frame_size] -> codes i64 [batch,num_codebooks,n_frames]. */
int mmi_mimi_encode_step(mmi_mimi* m, const float* pcm, int64_t* codes, int32_t batch, int32_t n_frames,
                         mmi_stream stream);
/* MimiModel.encode_to_latent(x, quantize=False) (compression.py:390-404):
 * pcm -> unquantized latent f32 [batch,dimension,n_frames]. */
int mmi_mimi_encode_latent_step(mmi_mimi* m, const float* pcm, float* latent, int32_t batch, int32_t n_frames,
                                mmi_stream stream);
/* SplitResidualVectorQuantizer.encode (vq.py:269-279) on a given latent (stateless):
 * latent f32 [batch,dimension,n_frames] -> codes i64 [batch,num_codebooks,n_frames]. */
int mmi_mimi_quantize(mmi_mimi* m, const float* latent, int64_t* codes, int32_t batch, int32_t n_frames,
                      mmi_stream stream);
/* MimiModel.decode_latent (compression.py:431-433; vq.py:281-287) (stateless):
 * codes i64 [batch,K,n_frames] -> latent f32 [batch,dimension,n_frames]. */
int mmi_mimi_decode_latent(mmi_mimi* m, const int64_t* codes, float* latent, int32_t batch, int32_t n_codebooks,
                           int32_t n_frames, mmi_stream stream);
/* MimiModel.decode in streaming mode (compression.py:406-429):
 * codes i64 [batch,K,n_frames] (values in [0,bins)) -> pcm f32 [batch,1,n_frames*frame_size]. */
int mmi_mimi_decode_step(mmi_mimi* m, const int64_t* codes, float* pcm, int32_t batch, int32_t n_codebooks,
                         int32_t n_frames, mmi_stream stream);
/* The same for a strided view: codes[b * batch_stride + k * n_frames + f].  What `mimi.decode(tokens[:, 1:])` is in the
 * reference's serving loop (server.py:144-146: the audio columns of LMGen.step's [B, 1 + dep_q, 1] output) - the view is read
 * in place, batch_stride = (1 + dep_q) * n_frames there. */
int mmi_mimi_decode_step_strided(mmi_mimi* m, const int64_t* codes, int64_t batch_stride, float* pcm, int32_t batch,
                                 int32_t n_codebooks, int32_t n_frames, mmi_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* Moshi LM (Temporal + Depth transformer) and LMGen                                          */
/* ------------------------------------------------------------------------------------------ */

/* Mirrors loaders._lm_kwargs (loaders.py:90-119) for the options LMGen.step exercises on Moshi.
 * Fixed by the kernels: norm "rms_norm_f32" (eps 1e-8), gating "silu", positional_embedding "rope"
 * (interleaved) for the temporal transformer and "none" for the depformer, causal, no fuser / no CFG,
 * depformer_multi_linear + depformer_weights_per_step, kv_repeat 1. */
typedef struct mmi_lm_cfg {
    int32_t dim;            /* 4096 */
    int32_t num_heads;      /* 32 */
    int32_t num_layers;     /* 32 */
    int32_t ffn_hidden;     /* gating hidden size: 11264 (gating.py:55-58) */
    int32_t context;        /* 3000 */
    float max_period;       /* 10000 */
    int32_t n_q;            /* 16 audio streams seen by the temporal transformer */
    int32_t dep_q;          /* 8 generated by the depformer */
    int32_t card;           /* 2048 */
    int32_t text_card;      /* 32000 */
    int32_t text_card_out;  /* 32000 */
    int32_t depformer_dim;        /* 1024 */
    int32_t depformer_num_heads;  /* 16 */
    int32_t depformer_num_layers; /* 6 */
    int32_t depformer_ffn_hidden; /* 2816 */
    int32_t delays[64];     /* num_codebooks = n_q + 1 entries (text first) */
    int32_t existing_text_padding_id; /* 3 */
    int32_t extra_heads_num_heads;    /* 0: nn.Linear(dim, extra_heads_dim) heads on the transformer output (lm.py:101-102, 224-226) */
    int32_t extra_heads_dim;          /* 6 */
    int32_t kv_cache_dtype;           /* 0 / MMI_BF16: the reference's bf16 ring (transformer.py:453-455); MMI_F8E4M3: e4m3 ring -
                                         half the attention stream and half the per-session state (SURVEY.md 8d C5 "fp8 KV");
                                         MMI_F4E2M1X2: 4-bit ring, 0.5625 bytes per element: E2M1 codes (bit 3 sign,
                                         bits 2..0 the magnitude of {0, .5, 1, 1.5, 2, 3, 4, 6}; two per byte, element 2i in the low
                                         nibble) under one E8M0 scale byte 2^(s - 127) per block of 16 consecutive head-dim elements of
                                         one (row, head, position).  Quantised: what the bf16 ring would hold (k after RoPE).  s = E - 2
                                         (E: biased exponent of the block's absmax), at most 253; E < 3: s = 0 and all codes 0; round to
                                         nearest, ties to the even code, saturating at +-6; Inf and NaN become +-6 under their sign.  Per
                                         layer, for keys and for values: a codes plane [B][H][cap][Dh/2] bytes, then a scale plane
                                         [B][H][cap][Dh/16] bytes (the layer padded to a multiple of 256 bytes).  Needs a head dim multiple of 32 (else MMI_ERR_UNSUPPORTED).  The
                                         depth transformer's cache and the cross-attention K/V stay bf16 */
    int32_t cross_attention;          /* 1: every temporal layer has a cross-attention block (`cross_attention.{in,out}_projs.0`,
                                         `norm_cross.{weight,bias}`; transformer.py:727-732, 779-786) fed by mmi_guidance.condition_cross */
} mmi_lm_cfg;

/* LMGen constructor arguments that change what step computes (lm.py:557-574). */
typedef struct mmi_sampling {
    int32_t use_sampling; /* 0 = greedy argmax */
    float temp;           /* audio temperature 0.8 */
    float temp_text;      /* 0.7 */
    int32_t top_k;        /* 250 */
    int32_t top_k_text;   /* 25 */
    uint64_t seed;        /* seed of the on-device counter RNG used when no noise is supplied */
} mmi_sampling;

typedef struct mmi_lm mmi_lm;

/* loaders.get_moshi_lm (loaders.py:366-446): build LMModel from state-dict tensors - bf16, or with the linears in the
 * reference's quantised storage (utils/quantize.py:13-22): `<linear>.weight` MMI_I8 [out,in] row-wise absmax codes plus
 * `<linear>.weight_scb` MMI_F32 [out] row absmax; or as fp8 (BASELINE configs[4], run on the fp8 MFMA): `<linear>.weight`
 * MMI_F8E4M3 [out,in] codes, `<linear>.weight_scale` MMI_F32 [out] (W ~= code * scale) and an optional scalar
 * `<linear>.input_scale` MMI_F32 (static activation scale: x8 = e4m3(x / input_scale), default 1).  Embeddings and norms
 * stay bf16.  The linears must be all bf16, all int8 or all fp8.
 * Or as OCP MXFP4 (Microscaling v1.0; weight-only, widened to bf16 inside the GEMM by v_cvt_scalef32_pk_bf16_fp4 - exact, so
 * the engine computes what the bf16 engine computes on the dequantised weights): `<linear>.weight` MMI_F4E2M1X2 [out, in/2],
 * two E2M1 codes per byte (element 2i in the low nibble; bit 3 sign, bits 2..0 magnitude of {0, 0.5, 1, 1.5, 2, 3, 4, 6}),
 * and `<linear>.weight_scale_e8m0` MMI_E8M0 [out, in/32], one scale 2^(s-127) per 32 consecutive input features of a row.
 * Refused, before anything is uploaded: in_features not a multiple of 32 (MMI_ERR_UNSUPPORTED), a missing or mis-shaped scale
 * tensor (MMI_ERR_MISSING_WEIGHT / MMI_ERR_SHAPE), a scale byte 255 - the E8M0 NaN - (MMI_ERR_INVALID), scale bytes outside
 * 2..252 (MMI_ERR_UNSUPPORTED: every dequantised weight stays a normal, finite bf16), other quantised widths next to it,
 * cross-attention layers, low-rank or demuxed embeddings, and more than 64 model rows (MMI_ERR_UNSUPPORTED). */
int mmi_lm_create(const mmi_lm_cfg* cfg, const mmi_tensor_desc* weights, int32_t n_weights,
                  int32_t max_batch, mmi_lm** out);

/* Options of the TTS-family LMs (kyutai's TTS checkpoints), next to mmi_lm_cfg so that its layout stays that of ABI version 3.
 * All zero = the model mmi_lm_create builds. */
struct mmi_lm_cfg_ext {
    /* depformer_weights_per_step_schedule (models/lm.py:125-127, 174-179; modules/transformer.py:291-318, 395-401, 684-688):
     * micro-step k runs the depformer weight set schedule[k] - `depformer_in.{w}`, `depformer.layers.*.self_attn.{in,out}_projs.{w}`
     * and `depformer.layers.*.gating.{w}` exist for w = 0..max(schedule) (values without gaps), `linears.{k}` for every k.
     * depformer_schedule_len: 0 = none (one set per step), else dep_q. */
    int32_t depformer_schedule[64];
    int32_t depformer_schedule_len;
    /* depformer_low_rank_embeddings (models/lm.py:180; models/lm_utils.py:80-94, 117-124): `depformer_emb.{k}.weight` [card+1, r]
     * and `depformer_text_emb.weight` [text_card+1, r], each followed by `<name>.low_rank.weight` [depformer_dim, r].  The
     * tables are expanded once at create, bf16(E @ low_rank^T) with fp32 sums, and gathered like full-rank ones.  0 = none. */
    int32_t depformer_low_rank;
    /* demux_second_text_stream (models/lm.py:135-139, 190-194; models/lm_utils.py:95-116; models/loaders.py:395-396): a text token
     * t is the pair (t % (text_card+1), t / (text_card+1) - 1) and embeds as bf16(out1(E[first]) + (second >= 0 ? out2(E[second]) : 0))
     * for `text_emb` ([dim, dim] `out1` / `out2`) and `depformer_text_emb` ([depformer_dim, r or depformer_dim]); out1(E) and out2(E)
     * are expanded once at create.  Needs depformer_dim to be a multiple of the 16- / 32-row tile. */
    int32_t demux_second_text_stream;
};
typedef struct mmi_lm_cfg_ext mmi_lm_cfg_ext;

/* mmi_lm_create with the options above; ext == NULL is mmi_lm_create.  Linears must be bf16 when low-rank or demuxed embeddings
 * are used.  dep_q up to 32, n_q == dep_q allowed (no user audio stream: mmi_lm_step takes n_user = 0). */
int mmi_lm_create_ext(const mmi_lm_cfg* cfg, const mmi_lm_cfg_ext* ext, const mmi_tensor_desc* weights, int32_t n_weights,
                      int32_t max_batch, mmi_lm** out);
/* A handle of up to 128 MODEL rows (sessions, or two rows per guided session).  mmi_lm_create / mmi_lm_create_ext refuse
 * max_batch > 64; this call takes max_rows 65..128 (ext may be NULL): the step's linears then run on k_gemm_rows, three or four
 * batch tiles of 32 in one pass over the weights, norms as separate launches.  max_rows <= 64 is mmi_lm_create_ext: the same
 * launch lists and the same bits.  Refused above 64 rows with MMI_ERR_UNSUPPORTED: int8 / fp8 linears; max_rows > 128.  Everything
 * downstream (streaming_start, the per-row calls, snapshots, mmi_lm_debug_linear, mmi_batcher_create) follows the handle's value. */
int mmi_lm_create_rows(const mmi_lm_cfg* cfg, const mmi_lm_cfg_ext* ext_or_null, const mmi_tensor_desc* weights, int32_t n_weights,
                       int32_t max_rows, mmi_lm** out);
void mmi_lm_destroy(mmi_lm* lm);

/* LMGen.streaming(batch) enter/exit (lm.py:605-666). */
int mmi_lm_streaming_start(mmi_lm* lm, int32_t batch, const mmi_sampling* sampling, mmi_stream stream);
/* LMGen's classifier-free guidance and conditioning arguments (lm.py:566-574, 612-651).  With
 * cfg_coef != 1 the model runs two rows per session (conditioned, unconditioned) - 2 * batch must fit max_batch - and every
 * sampling site draws from logits_null + (logits - logits_null) * cfg_coef (lm.py:727-733, 828-832).
 *   cfg_is_masked_until  host i64 [batch] or NULL: the unconditioned row reads zero tokens until offset > delay + value (lm.py:713-721)
 *   cfg_is_no_text       the unconditioned row never reads text tokens and the text logits stay unguided (lm.py:724-732)
 *   condition_sum        device bf16 [model rows, dim] or NULL: ConditionFuser.get_sum of the condition tensors, added to the
 *                        input embeddings of every step (lm.py:621-628, 399-400); model rows = batch, or 2 * batch when guided
 *                        (conditioned rows first).
 *   condition_cross      device bf16 [model rows, cross_len, dim] or NULL: ConditionFuser.get_cross of the condition tensors
 *                        (conditioners/base.py:392-409), the source of every temporal layer's cross-attention block; required
 *                        when the model was created with cfg.cross_attention.  Its keys / values are projected once, here
 *                        (the reference caches them on the first step, transformer.py:521-531). */
typedef struct mmi_guidance {
    float cfg_coef;
    int32_t cfg_is_no_text;
    const int64_t* cfg_is_masked_until;
    const void* condition_sum;
    const void* condition_cross;
    int32_t cross_len;
} mmi_guidance;
int mmi_lm_streaming_start_guided(mmi_lm* lm, int32_t batch, const mmi_sampling* sampling, const mmi_guidance* guide_or_null,
                                  mmi_stream stream);
int mmi_lm_model_rows(const mmi_lm* lm);
/* Sessions of the current stream (rows of the caller's tensors); 0 when not streaming. */
int mmi_lm_streaming_batch(const mmi_lm* lm);
/* A handle binds to the HIP device that is current when it is created (weights, state, streams and graphs live there); every
 * entry point switches the calling thread to that device for the call and restores the caller's.  Pointers passed in must be
 * on that device.  mmi_*_device return the ordinal. */
int mmi_lm_device(const mmi_lm* lm);
int mmi_mimi_device(const mmi_mimi* m);
/* Engine counters for tests / diagnostics.  which = 0: GEMM launches (or captured graph nodes) that took the LDS-resident
 * kernel (k_gemm_xlds); 1: bit v set = step program v (short-ring / deep-ring decode attention) is captured and instantiated -
 * both are from the stream's first step on, so that the switch is never a capture inside a live session; 2: the host's bound on
 * the ring depth (steps since streaming_start / seek / the offsets of a restored snapshot); 3: the depth transformer's MFMA tile
 * (16 at <= 32 sessions with bf16 weights, else 32); 4: GEMM launches (or captured graph nodes) that took k_gemm_rows (more
 * than 64 model rows).  0 and 4 count the GEMMs of mmi_lm_prefill passes as well as those of steps. */
int64_t mmi_lm_stat(const mmi_lm* lm, int32_t which);
/* LMGen.step_with_extra_heads (lm.py:793-807): softmax(extra_head(transformer_out)) of the LAST step for every head:
 * probs f32 [model rows, extra_heads_num_heads, extra_heads_dim]. */
int mmi_lm_extra_heads(mmi_lm* lm, float* probs, mmi_stream stream);
/* get / set_streaming_state of LMGen (streaming.py:158-181; _LMGenState lm.py:520-547): KV rings, token ring, offsets, masks,
 * RNG counter as one opaque device buffer; host_word carries the host-side step counter (`offset_cpu`). */
int64_t mmi_lm_state_bytes(const mmi_lm* lm);
int mmi_lm_state_save(mmi_lm* lm, void* dst, int64_t bytes, int64_t* host_word, mmi_stream stream);
int mmi_lm_state_load(mmi_lm* lm, const void* src, int64_t bytes, int64_t host_word, mmi_stream stream);
int mmi_lm_streaming_stop(mmi_lm* lm);
int mmi_lm_set_exec_mask(mmi_lm* lm, const uint8_t* mask, mmi_stream stream);        /* lm.py:544-547 */
int mmi_lm_reset(mmi_lm* lm, const uint8_t* mask_or_null, mmi_stream stream);        /* lm.py:537-542 */
/* Fork session `src` into the sessions dst[0 .. n_dst) of the same stream (dst: a host array): a parked template session copied
 * at admission instead of a prefill per caller, or N candidates continued from one conversation state.  No reference
 * counterpart: the nearest is get_streaming_state / set_streaming_state on a batch of one (streaming.py:158-181).
 * Stream-ordered: no host synchronisation and no device read-back; only the valid rows of the source's KV ring are moved (their
 * number is read on the device).  After the call each destination is the session `src` is: offset, delay ring, last tokens,
 * text history, sampling entry (a seeded draw stream continues with the same draws: set another mmi_row_sampling afterwards for
 * different candidates), top_p, condition rows and guidance coefficient, cross-attention source and length, TTS script position,
 * adapter slot; on a guided stream the twin model rows follow.  A destination's previous state is gone as after mmi_lm_reset,
 * its exec bit is 1 whatever the source's is, and its rows of the log-probability rings are cleared as mmi_lm_reset clears
 * them.  The handle-wide RNG counter, the host step counter and the ring-depth bound stay as they are.  Works on every handle
 * mmi_lm_step works on.  MMI_ERR_STATE when not streaming; MMI_ERR_INVALID for src or a dst outside [0, batch), dst == src, a
 * repeated dst, n_dst outside [1, 16]; a refused call changes nothing. */
int mmi_lm_fork_session(mmi_lm* lm, int32_t src, const int32_t* dst, int32_t n_dst, mmi_stream stream);

/* Per-session sampling settings (no counterpart in the reference's Python LMGen; its Rust server takes them from each
 * connection's query string, rust/moshi-backend/src/stream_both.rs:95-105, and applies them to that session alone,
 * rust/moshi-core/src/lm_generate_multistream.rs:142-183, 247-255).  A session that has an entry samples every site with its own
 * values and its own Philox stream: key = seed, counter (the session's stream offset, site, entry) - so its draws do not depend
 * on its slot, on the batch size or on how many steps the handle has run, and on a fresh stream they are the draws of a
 * one-session stream started with the same mmi_sampling.  The text site of such a session also gets, in this order:
 *   repetition penalty  every distinct token among the newest repetition_context entries of the session's ring of its last 64
 *                       committed text tokens (the token the step stores, after forcing and hooks; the padding id, the
 *                       end-of-padding id (0 unless mmi_lm_set_text_end_padding_id moved it) and the text start id are never
 *                       recorded; masked steps record nothing) has its logit changed: l >= 0 ? l / penalty : l * penalty - fp32 from the bf16 logit, correctly rounded division,
 *                       rounded back to bf16 (nearest even).  Ids outside the vocabulary are ignored.
 *   pad bias            sampling sessions only (greedy ones ignore it, like the reference's ArgMax): the logit of
 *                       existing_text_padding_id becomes bf16(l + pad_mult * temp_text), an fp32 product then an fp32 sum - the
 *                       reference's prs[pad] *= exp(pad_mult) after the temperature softmax, in logit space.  Its resolution is
 *                       one bf16 ulp of the pad logit: a bias smaller than half an ulp leaves the row unchanged.
 * Both come after the guidance mix and after an on_text_logits hook.  Sessions without an entry sample exactly as before. */
struct mmi_row_sampling {
    int32_t use_sampling;        /* 0 = greedy argmax                                  */
    float temp;                  /* audio temperature                                  */
    float temp_text;
    int32_t top_k;               /* 0 (or >= the vocabulary) = the full multinomial    */
    int32_t top_k_text;
    uint64_t seed;               /* one seed per session: text and audio sites share it */
    float pad_mult;              /* 0 = off                                            */
    float repetition_penalty;    /* 1 = off; must be > 0                               */
    int32_t repetition_context;  /* 0 = off; at most 64                                */
};
typedef struct mmi_row_sampling mmi_row_sampling;
/* MMI_OK, or what mmi_lm_set_row_sampling would refuse the entry with: top_k / top_k_text > 256 MMI_ERR_UNSUPPORTED, < 0
 * MMI_ERR_INVALID (as for mmi_sampling); repetition_context outside [0, 64], repetition_penalty <= 0 or any non-finite value
 * MMI_ERR_INVALID. */
int mmi_row_sampling_check(const mmi_row_sampling* r);
/* The sessions b with mask[b] != 0 (mask: HOST uint8 [batch], NULL = all) take rows[b] (HOST [batch]; entries of unmasked
 * sessions are not read), their ring of text tokens is emptied and they sample with their own settings from the next step on.
 * Stream-ordered on `stream`, no host synchronisation (the entries travel as kernel arguments), legal between any two steps;
 * neither the launch list nor a captured graph changes.  Under guidance it addresses sessions, not model rows.  A refused call
 * changes nothing.  mmi_lm_reset keeps a session's settings and empties its ring; streaming_start begins with no entries; a state
 * snapshot carries entries and rings.  While any session has an entry, mmi_lm_step refuses opt_noise (MMI_ERR_UNSUPPORTED). */
int mmi_lm_set_row_sampling(mmi_lm* lm, const uint8_t* mask_or_null, const mmi_row_sampling* rows, mmi_stream stream);
/* The masked sessions (HOST uint8 [batch], NULL = all) return to the handle's mmi_sampling and the handle's counter. */
int mmi_lm_clear_row_sampling(mmi_lm* lm, const uint8_t* mask_or_null, mmi_stream stream);
/* The end-of-padding id the text history skips (the reference's text_eop_token; LMModel.end_of_text_padding_id, which a
 * checkpoint's existing_text_end_padding_id may move).  0 after create.  Not while streaming (MMI_ERR_STATE): the id is an
 * argument of the commit kernel in the launch list.  An id outside [0, text_card] is MMI_ERR_INVALID. */
int mmi_lm_set_text_end_padding_id(mmi_lm* lm, int32_t id);

/* Per-session conditions and guidance strength (no counterpart in the reference's Python LMGen, which fixes them for the whole
 * stream, lm.py:612-651; its Rust TTS server takes the voice's cross-attention source and the guidance strength from each
 * request's query: rust/moshi-server/src/tts.rs:342-357).  A session of a live stream gets its own `sum` condition row, its own cross-attention source with its own length
 * and its own guidance coefficient; under guidance a session is two model rows (b and batch + b) and the call fans out to the
 * twin itself.
 *   cfg_coef         1 = this session's sampling sites keep the conditioned logits untouched (the reference does not mix at 1,
 *                    lm.py:727); != 1 only on a stream that was started with guidance (it has the twin rows)
 *   condition_sum    device bf16 [R, dim] or NULL = keep; R = 1, or 2 on a guided stream (conditioned row first); only on a
 *                    stream started with a condition_sum (it has the buffer)
 *   condition_cross  device bf16 [R, cross_len, dim] or NULL = keep: projected through every temporal layer's key / value rows
 *                    into the session's own slots, the same bits mmi_lm_streaming_start_guided gives the same positions
 *   cross_len        1 .. capacity; read only with condition_cross.  Positions beyond a row's length are never read. */
struct mmi_row_condition {
    float cfg_coef;
    const void* condition_sum;
    const void* condition_cross;
    int32_t cross_len;
};
typedef struct mmi_row_condition mmi_row_condition;
/* Positions a row's cross-attention source may hold in the streams started after this call (the keys / values buffer of the
 * streaming state is [layers][model rows][capacity][2 dim], so mmi_lm_state_bytes grows with it).  0 (the default) = the
 * cross_len given at streaming_start, as before.  Not while streaming (MMI_ERR_STATE).  A streaming_start whose cross_len
 * exceeds a capacity set here is refused with MMI_ERR_SHAPE.  mmi_lm_cross_capacity: the capacity of the live stream, or the
 * value set here when not streaming (a negative status for a NULL handle). */
int mmi_lm_set_cross_capacity(mmi_lm* lm, int32_t positions);
int mmi_lm_cross_capacity(const mmi_lm* lm);
/* Session `session` takes the condition *c from its next step on.  Stream-ordered on `stream`, no host synchronisation (the
 * scalars travel as kernel arguments, the projection is enqueued), legal between any two steps; neither the launch list nor a
 * captured graph changes.  The device buffers c names must stay valid until `stream` has passed the call.  streaming_start sets
 * every session from mmi_guidance; mmi_lm_reset keeps a session's condition; a state snapshot carries conditions, lengths and
 * coefficients.  Hooks, supplied noise and forced tokens are unaffected.  A refused call changes nothing: not streaming
 * MMI_ERR_STATE; session outside [0, batch) or a non-finite cfg_coef MMI_ERR_INVALID; cfg_coef != 1 on a stream started without
 * guidance, or condition_sum on a stream started without one, MMI_ERR_STATE; condition_cross on a model without
 * cross-attention layers MMI_ERR_INVALID; cross_len outside [1, capacity] MMI_ERR_SHAPE. */
int mmi_lm_set_row_condition(mmi_lm* lm, int32_t session, const mmi_row_condition* c, mmi_stream stream);

/* ---- per-session LoRA adapters, unmerged, on one base model (modules/lora.py; loaders.py:486-516) ------------------------------
 * The reference runs a LoRA fine-tune either merged (fuse_lora=True: W' = W + scaling * B A, what a caller gets by merging before
 * mmi_lm_create) or unmerged: frozen_W(x) + lora_B(lora_A(x)) * scaling (lora.py:116-118).  An adapter handle keeps up to
 * max_adapters adapters of rank <= max_rank NEXT TO one base model and runs every model row with the adapter of its session:
 *   t = bf16(A x)   (a shrink launch in front of every linear: lora_A's bf16 output)
 *   out = epilogue(W x + bf16(scaling * B) t)   (one fp32 accumulator inside the linear's own GEMM)
 * Adapted: every nn.Linear the reference wraps - the four linears of every temporal and depth-transformer layer, depformer_in.{k},
 * text_linear, linears.{k}.
 *
 * mmi_lm_enable_adapters: before streaming_start (like mmi_lm_enable_tts_machine); allocates the zeroed banks.  max_adapters 1..8,
 * max_rank 32 / 64 / 96 / 128; (0, 0) turns adapters off again and frees the banks.  MMI_ERR_UNSUPPORTED, with the reason: quantised
 * linears of any width, more than 64 model rows, cross-attention layers, extra heads, low-rank or demuxed embeddings (the
 * reference wraps their linears too), the depth transformer on its own tile (MMI_DEP_TILE), a handle that is streaming.  A handle that never calls it is unchanged: same launch list, same bits, same mmi_lm_state_bytes. */
int mmi_lm_enable_adapters(mmi_lm* lm, int32_t max_adapters, int32_t max_rank);
/* Adapter `slot` = the bf16 DEVICE tensors `<linear>.lora_A.weight` [r, in] and `<linear>.lora_B.weight` [out, r] (names as the
 * engine's own weights, un-fused per step; `<linear>.frozen_W.weight` entries are ignored).  Checked before anything is written
 * (MMI_ERR_INVALID): r a multiple of 8 and <= max_rank, shapes fit the base linear, every A has its B, no unknown keys
 * (loaders.py:508-511), every value finite - scaling * lora_B in bf16 included.  A linear the adapter does not mention keeps
 * zero columns.  bf16(scaling * B) is formed here, exact for the reference's default scaling 2 and any power of two.  Allowed
 * while streaming, ordered on `stream` (which it synchronises once, for the check); MMI_ERR_STATE while a live session runs on
 * the slot. */
int mmi_lm_load_adapter(mmi_lm* lm, int32_t slot, float scaling, const mmi_tensor_desc* tensors, int32_t n_tensors, mmi_stream stream);
/* Zeroes the slot, under the same rule. */
int mmi_lm_unload_adapter(mmi_lm* lm, int32_t slot, mmi_stream stream);
/* Session `session` (both model rows of a guided one) runs on adapter `slot` (-1 = none) from the next step on.  Stream ordered;
 * the launch list and a captured step graph stay as they are.  streaming_start sets every session to -1; mmi_lm_reset leaves the
 * slot alone, an exec mask does not apply; mmi_lm_state_save / load carry the table. */
int mmi_lm_set_row_adapter(mmi_lm* lm, int32_t session, int32_t slot_or_minus1, mmi_stream stream);
/* The session's slot; -1: none (also without adapters, outside a stream or for a session outside the batch). */
int32_t mmi_lm_row_adapter(const mmi_lm* lm, int32_t session);

/* ---- nucleus (top-p) sampling, per handle and per session (utils/sampling.py:67-83, 97-98) ----------------------
 * A sampling site whose effective top_p is p, 0 < p <= 1, draws from the nucleus of its final bf16 logit row (behind the
 * guidance mix, an on_text_logits hook, the TTS padding bonus, the repetition penalty and the pad bias): with the entries ordered
 * by (logit descending, index ascending) and P = softmax(logits / temp) in fp32, the entry of rank r is in iff the mass of the
 * ranks before it is <= p (the reference's `probs_sum - probs_sort > p` mask; equality keeps the entry; rank 0 is always in).
 * top_p > 0 overrides the site's top_k, as in the reference; greedy rows and rows with temp <= 0 ignore it; p = 1 is the whole
 * vocabulary; p = 0 is off (exactly the bits of before).  The winner is drawn as the top-k path draws it: member i scores
 * logit_i / temp - log(-log u_i), u_i from the session's (or the handle's) Philox stream at (step, site, i); the largest score
 * wins, ties to the lower index - so a nucleus of n <= 256 members yields the token top_k = n yields on the same stream.  The
 * masses are fp32 sums in a fixed order: the same set on every run.  The set may differ from a sequential fp32 cumsum's only
 * where a prefix mass lies within summation error of p.
 *
 * mmi_lm_enable_nucleus: the next streaming_start builds its launch list on the nucleus forms of the three samplers (any kind of
 * handle).  MMI_ERR_STATE while streaming, or when turning it off while the handle's top_p is positive.  A handle that never
 * calls it is unchanged: same launch list, same device code, same mmi_lm_state_bytes.  An enabled stream's snapshot grows by
 * 8 bytes per session, rounded up to 48. */
int mmi_lm_enable_nucleus(mmi_lm* lm, int32_t on);
/* The handle-wide (audio sites, text site) values; they stay until changed and every session of the next streaming_start begins
 * with them.  MMI_ERR_STATE while streaming, and for a non-zero value on a handle without the nucleus samplers; values outside
 * [0, 1] or non-finite MMI_ERR_INVALID.  A refused call changes nothing. */
int mmi_lm_set_top_p(mmi_lm* lm, float top_p, float top_p_text);
int mmi_lm_top_p(const mmi_lm* lm, float* top_p, float* top_p_text);
/* 1: the live stream runs the nucleus samplers (not streaming: the next one will); 0: not; a negative status for a NULL handle. */
int32_t mmi_lm_nucleus_enabled(const mmi_lm* lm);
/* Session `session` samples with its own (top_p, top_p_text) from the next step on / returns to the handle's.  Stream ordered (the
 * values travel as kernel arguments), legal between any two steps; neither the launch list nor a captured graph changes.  Under
 * guidance they address sessions.  Independent of whether the session has an mmi_row_sampling entry.  mmi_lm_reset keeps the
 * values; a state snapshot carries them.  MMI_ERR_STATE when not streaming or on a stream started without the nucleus samplers;
 * session outside [0, batch) or a value outside [0, 1] MMI_ERR_INVALID.  While the handle's or any session's value is positive,
 * mmi_lm_step refuses opt_noise (MMI_ERR_UNSUPPORTED; nothing is enqueued): rank-indexed draws over a nucleus are not built. */
int mmi_lm_set_row_top_p(mmi_lm* lm, int32_t session, float top_p, float top_p_text, mmi_stream stream);
int mmi_lm_clear_row_top_p(mmi_lm* lm, int32_t session, mmi_stream stream);

/* The TTS script machine on the device: what TTSModel.generate's three host hooks do on every frame
 * (models/tts.py:553-583) - StateMachine.process per row (tts.py:160-252), the zeroed / prefixed audio codebooks, the padding
 * bonus - as part of the launch list, so that a TTS step stays one captured graph.  The fields are StateMachine's and
 * TTSModel's: text_card = TokenIds.card (the mux base of a demuxed text stream: the model's text_card + 1), new_word, pad, zero
 * (tts.py:37-57; zero must be -1), second_stream_ahead, max_padding, initial_padding (tts.py:146-149), delay_steps and
 * padding_bonus (tts.py:563, 555). */
struct mmi_tts_params {
    int32_t text_card, new_word, pad, zero;
    int32_t second_stream_ahead, max_padding, initial_padding, delay_steps;
    float padding_bonus;
};
typedef struct mmi_tts_params mmi_tts_params;
/* Replaces LMGen(on_text_logits_hook, on_text_hook, on_audio_hook) of tts.py:588-593 for the streams started after the call, in
 * the manner of mmi_lm_set_cross_capacity: a property of the handle, not while streaming (MMI_ERR_STATE).  Capacities per
 * session: script entries, script tokens, prefix columns (they size the machine's rows in the streaming state, which
 * mmi_lm_state_save / _load carry).  The step then runs k_tts_machine behind the text sampler (on a demuxed model in place of the
 * launch that wrote the depth transformer's first input row, else as one added launch), applies the audio rule in the ring
 * commit and the padding bonus in the text sampler.  NULL params: off again - the launch list of a handle that never enabled it.
 * Refused: dep_q == 0, or second_stream_ahead > 0 on a model without a demuxed text stream, MMI_ERR_UNSUPPORTED; negative
 * values, ids outside the text vocabulary, zero != -1, a mux base that is not text_card + 1 MMI_ERR_INVALID. */
int mmi_lm_enable_tts_machine(mmi_lm* lm, const mmi_tts_params* params, int32_t max_entries, int32_t max_tokens, int32_t max_prefix);
/* One session's script: HOST arrays, copied by the call.  Entry e (tts.py:60-74 Entry) owns tokens[entry_first[e] ..
 * entry_first[e + 1]) - none = a break - and entry_padding[e]; entry_first has n_entries + 1 values, the first 0.
 * text_prefix [text_prefix_len] and audio_prefix [dep_q][audio_prefix_len] are row 0 and rows audio_offset.. of
 * generate(prefixes=...) (tts.py:536-551), un-delayed: the engine delays each codebook by its delay + delay_steps as `_delayed`
 * does; -2 (ungenerated) entries leave the sampled token. */
struct mmi_tts_script {
    const int32_t* tokens;
    const int32_t* entry_first;
    const int32_t* entry_padding;
    int32_t n_entries;
    const int32_t* text_prefix;
    int32_t text_prefix_len;
    const int32_t* audio_prefix;
    int32_t audio_prefix_len;
};
typedef struct mmi_tts_script mmi_tts_script;
/* Session `session` runs `script` from `new_state` (tts.py:151-158, 530) from its next step on; NULL: no script, its sampled text
 * token passes through.  Stream-ordered like k_lm_set_rows: the row is composed in pinned memory and copied on `stream`, no host
 * synchronisation; neither the launch list nor a captured graph changes and no other session is touched.  The machine's step
 * index is the session's own stream offset (mmi_lm_seek / reset), so a session that starts later in a live batch behaves like a
 * fresh stream; with all rows in step it is the loop index of tts.py:602.  mmi_lm_reset of the row rewinds its machine to
 * new_state of the same script (as it keeps the row's condition and sampling settings).  Appending entries to a running script is
 * not built: a call replaces the script.  A refused call changes nothing: machine not enabled or not streaming MMI_ERR_STATE;
 * session outside [0, batch), a token outside the text vocabulary, a negative padding MMI_ERR_INVALID; more entries, tokens or
 * prefix columns than the capacities MMI_ERR_SHAPE. */
int mmi_lm_set_row_script(mmi_lm* lm, int32_t session, const mmi_tts_script* script, mmi_stream stream);
/* TTSResult's end_steps / all_consumption_times of one session (tts.py:624-628; end_step -1 = None).  consumption_times: HOST
 * [capacity] or NULL; the first min(n_consumed, capacity) values are written.  Waits for `stream`. */
struct mmi_tts_status {
    int32_t has_script, end_step, n_consumed;
    int32_t* consumption_times;
    int32_t capacity;
};
typedef struct mmi_tts_status mmi_tts_status;
int mmi_lm_row_script_status(mmi_lm* lm, int32_t session, mmi_tts_status* out, mmi_stream stream);

/* LMGen.step (lm.py:785-791, 668-783).
 *   user_codes  i64 [batch, n_user(>= n_q - dep_q), 1]; extra rows are ignored (lm.py:688-689)
 *   out_tokens  i64 [batch, dep_q + 1, 1]; rows not yet valid hold -2 (lm.py:781-782)
 *   opt_text_logits  f32 [batch, text_card_out] or NULL   } parity taps: the logits the tokens were
 *   opt_audio_logits f32 [batch, dep_q, card]   or NULL   } sampled from (bf16 values widened to f32)
 *   opt_noise   f32 [batch, 1 + dep_q, max(top_k, top_k_text)] or NULL: Exp(1) draws used instead of the
 *               on-device RNG, indexed by rank in the descending top-k (sampling.py:40-47,59-63)
 *   valid (host int*): 0 while offset_cpu <= max_delay, i.e. where the reference returns None (lm.py:774-776)
 */
int mmi_lm_step(mmi_lm* lm, const int64_t* user_codes, int32_t n_user, int64_t* out_tokens,
                float* opt_text_logits, float* opt_audio_logits, const float* opt_noise, int32_t batch,
                int32_t* valid, mmi_stream stream);

/* Phase callback (no reference counterpart; used by the duplex pipeline below): a host function that every following
 * mmi_lm_step calls, on the calling thread, between the temporal transformer + text head (chip-filling, HBM-bound GEMMs) and
 * the depth transformer (dep_q x 33 small dependent launches that leave most CUs idle), with the step's stream: what it
 * enqueues there marks the point from which other streams can run beside the step without costing it.  A non-zero return
 * aborts the step.  NULL clears. */
int mmi_lm_set_phase_callback(mmi_lm* lm, int (*fn)(void* user, mmi_stream stream), void* user);

/* LMGen's per-step hooks (lm.py:568-570, 734-747): host callbacks between the stages of a step, each of which may READ and
 * MODIFY IN PLACE what the reference's hook receives (the TTS wrapper forces text tokens this way, models/tts.py):
 *   on_text_logits   after the (guided) text logits are final, before the text token is sampled      (lm.py:734-735)
 *   on_text_token    after the text token is sampled, before the depth transformer reads it          (lm.py:746-747)
 *   on_audio_tokens  after the dep_q audio tokens are sampled (or replaced), before they enter the ring (lm.py:756-757)
 * With any hook set, mmi_lm_step launches the step in segments (no graph replay) on `stream` and calls the hooks on the
 * calling thread, without synchronising: a hook works on the same stream through mmi_lm_hook_io.  A non-zero return aborts the
 * step with MMI_ERR_INVALID.  Pass NULL to clear. */
typedef struct mmi_lm_hooks {
    int (*on_text_logits)(void* user);
    int (*on_text_token)(void* user);
    int (*on_audio_tokens)(void* user);
    void* user;
} mmi_lm_hooks;
int mmi_lm_set_hooks(mmi_lm* lm, const mmi_lm_hooks* hooks_or_null);
/* Inside a hook: copy one of the step's tensors out (write = 0) or back in (write = 1), stream-ordered on `stream`:
 *   which 0  text logits   bf16 [batch, text_card_out]   (the model dtype, as the reference's hook sees them)
 *   which 1  text token    i64  [batch]
 *   which 2  audio tokens  i64  [batch, dep_q]
 * nbytes = the size of `buf`; anything but the tensor's size is refused (MMI_ERR_SHAPE). */
int mmi_lm_hook_io(mmi_lm* lm, int32_t which, int32_t write, void* buf, int64_t nbytes, mmi_stream stream);
int32_t mmi_lm_has_hooks(const mmi_lm* lm);         /* 1 while any of the three hooks is set */

/* Teacher forcing for the NEXT step only: tokens i64 [batch, 1 + dep_q] (text, then the dep_q audio codebooks);
 * entries >= 0 replace the sampled token at that site (the logits taps are still produced), entries < 0 keep
 * sampling.  Covers LMGen.step's `depformer_replace_tokens` argument (lm.py:751-755) and lets the parity tests
 * replay the reference's token history exactly. */
int mmi_lm_force_next_tokens(mmi_lm* lm, const int64_t* tokens, mmi_stream stream);

/* Parity tap of the residual stream (test aid; the reference has none - it is what a forward hook on
 * `transformer.layers[0]` / `layers[-1]` would see, transformer.py:814-929): switched on BEFORE streaming_start, every step also
 * keeps the hidden state after the first and after the last temporal layer; get copies bf16 [2][model rows][dim] (row-major)
 * out, stream-ordered.  Off by default: no launch is added. */
int mmi_lm_set_hidden_taps(mmi_lm* lm, int32_t on);
int mmi_lm_get_hidden_taps(mmi_lm* lm, void* buf_bf16, int64_t nbytes, mmi_stream stream);

/* Parity tap (test aid; no reference counterpart - it is `F.linear(x, weight)` / `QLinear.forward(x)` of ONE module,
 * utils/quantize.py:24-40, on rows the caller supplies): runs the linear stored under the state-dict key `weight_name`
 * ("transformer.layers.0.gating.linear_in.weight", "depformer.layers.2.self_attn.out_projs.5.weight", "linears.3.weight", ...)
 * through the kernels the step uses for it and returns its bf16 output, so that a test can hold the engine's int8 x int8
 * arithmetic to the oracle BIT FOR BIT, per linear, instead of through the logits of a whole network.
 *   x         device bf16 [rows][in_features], row-major; rows <= max_batch
 *   out       device bf16 [rows][out_features]; a gated linear_in returns [rows][hidden] = silu(gate) * value, what the step hands on
 *   path      MMI_DBG_PLAIN       (int8 x int8 models: k_quant_rows_i8, then) the weight-streaming GEMM as planned for the
 *                                 shape and batch (k_gemm_xp / k_gemm_xlds), store epilogue
 *             MMI_DBG_SPLITK      the same operand through the split-K form + the fold of the next norm launch
 *                                 (out = bf16(sum of the partials)); MMI_ERR_UNSUPPORTED if the engine does not split this GEMM
 *             MMI_DBG_FUSED       k_gemm_q8: the row quantisation inside the GEMM (int8 x int8 models, rows of <= 88 entries)
 *             MMI_DBG_NORM        RMSNorm with the vector stored under `alpha_name` first, as the step's norm launch does it
 *                                 (k_resid_rmsnorm + its int8 copy), then the GEMM; norm_out (optional, bf16 [rows][in_features])
 *                                 receives the normalised rows
 *             MMI_DBG_NORM_FUSED  the norm inside the GEMM (k_gemm_xp_norm / k_gemm_q8<NORM>; rows of <= 1024 features)
 *   codes, absmax (optional; int8 x int8 models, paths PLAIN / SPLITK / NORM): int8 [rows][in_features] and fp32 [rows] - the
 *             row-wise quantisation the GEMM consumed (bitsandbytes' CA / SCA)
 * Does not touch a running stream's state (own scratch); synchronises `stream`. */
enum { MMI_DBG_PLAIN = 0, MMI_DBG_SPLITK = 1, MMI_DBG_FUSED = 2, MMI_DBG_NORM = 3, MMI_DBG_NORM_FUSED = 4 };
int mmi_lm_debug_linear(mmi_lm* lm, const char* weight_name, const char* alpha_name_or_null, int32_t path, const void* x_bf16,
                        int32_t rows, void* out_bf16, int8_t* codes_or_null, float* absmax_or_null, void* norm_out_or_null,
                        mmi_stream stream);

/* mmi_lm_debug_linear on an adapter handle (mmi_lm_enable_adapters): the shrink launch plus the GEMM of that linear as the step
 * runs them, for rows whose adapter slots are row_slots[rows] (HOST int32, -1 = no adapter).  Paths MMI_DBG_PLAIN and
 * MMI_DBG_SPLITK (an adapter handle takes no fused form); out = bf16(W x + bf16(scaling * B) bf16(A x)) through the linear's
 * usual epilogue. */
int mmi_lm_debug_linear_lora(mmi_lm* lm, const char* weight_name, const char* alpha_name_or_null, int32_t path, const void* x_bf16,
                             int32_t rows, void* out_bf16, int8_t* codes_or_null, float* absmax_or_null, void* norm_out_or_null,
                             const int32_t* row_slots, mmi_stream stream);

/* Test aids of the KV ring (no reference counterpart).
 * mmi_lm_debug_kv4_quantize: the device quantiser of the 4-bit ring (mmi_lm_cfg.kv_cache_dtype = MMI_F4E2M1X2) on caller-supplied
 *   rows: x device bf16 [n][16 * m] -> codes device u8 [n][8 * m] and scales device u8 [n][m], block j of a row = its elements
 *   16 j .. 16 j + 15.  x must be 16-byte aligned and codes 8-byte aligned (vector loads and stores).  Works on any handle (it
 *   touches no state); synchronises `stream`.
 * mmi_lm_debug_kv_ring: the raw ring bytes of temporal layer `layer` (which = 0 keys, 1 values) of a live stream, copied to the
 *   device buffer `dst` of exactly mmi_lm_debug_kv_ring(.., dst = NULL, ..) bytes - that call returns the size and copies nothing.
 *   bf16 ring: [rows][H][cap][Dh] bf16; e4m3: the same in bytes; 4-bit: the codes plane [rows][H][cap][Dh/2], then the scale plane
 *   [rows][H][cap][Dh/16] (rows = model rows: sessions, then their guidance twins).  Returns the bytes copied, or a negative mmi_status. */
int mmi_lm_debug_kv4_quantize(mmi_lm* lm, const void* x_bf16, int32_t n, int32_t m, void* codes_u8, void* scales_u8, mmi_stream stream);
int64_t mmi_lm_debug_kv_ring(mmi_lm* lm, int32_t layer, int32_t which, void* dst, int64_t nbytes, mmi_stream stream);

/* Parity tap of the temporal decode attention (tests; no reference counterpart): the attention op of a temporal layer - the
 * launches the step makes for it, through the step's own dispatch - on caller-supplied operands, so that the kernels can be held
 * to an exact softmax on their own.  Works on any handle and touches no stream state: the partials, the (zeroed) arrival counters
 * and the packed output live in scratch of the call.  The caller sets everything a handle's model would otherwise fix:
 *   q        device bf16 [rows][H][Dh], taken as already roped (16-byte aligned)
 *   k, v     device bytes, the layout of mmi_lm_debug_kv_ring for a ring of `cap` slots (16-byte aligned): kv_dtype MMI_BF16
 *            [rows][H][cap][Dh] bf16, MMI_F8E4M3 the same in bytes, MMI_F4E2M1X2 the codes plane, then the scale plane
 *   offsets  device int64 [rows], >= 0: row b attends from position offsets[b], which sits in slot offsets[b] % cap
 *   H, Dh (32, 64 or 128), cap, context (1 <= context <= cap): context < cap is a ring longer than its attention window
 *   kernel   MMI_ATTN_WAVE (k_lm_attn_wave) or MMI_ATTN_SPLIT (k_lm_attn_split, the chunked kernel)
 *   NS       1 .. 16 workgroups per (row, head)
 *   merge    NS > 1: MMI_ATTN_MERGE_LAUNCH = every workgroup leaves its partial and k_lm_attn_combine follows (solo_rows is not
 *            read); MMI_ATTN_MERGE_KERNEL (k_lm_attn_wave only) = rings of at most solo_rows rows are walked by workgroup 0
 *            alone, deeper ones are merged by the workgroup that arrives last
 *   out      device bf16 [rows][H * Dh], row-major: unpacked from the packed activation layout that out_proj reads
 * Refuses (MMI_ERR_SHAPE / MMI_ERR_UNSUPPORTED) another head dim, rows above the handle's max_batch, a 4-bit ring whose head dim
 * is no multiple of 32, and operands aligned below what the vector loads need.  Synchronises `stream`. */
enum { MMI_ATTN_WAVE = 0, MMI_ATTN_SPLIT = 1 };
enum { MMI_ATTN_MERGE_LAUNCH = 0, MMI_ATTN_MERGE_KERNEL = 1 };
int mmi_lm_debug_attn(mmi_lm* lm, const void* q_bf16, const void* k_ring, const void* v_ring, const int64_t* offsets, int32_t rows,
                      int32_t H, int32_t Dh, int32_t cap, int32_t context, int32_t kv_dtype, int32_t kernel, int32_t NS, int32_t merge,
                      int32_t solo_rows, void* out_bf16, mmi_stream stream);

/* Parity taps of the depth transformer's attention and of the cross attention (tests; no reference counterpart):
 * the launch functions of the step - launch_dep_attn, which the scoring pass calls too, and launch_cross_attn - on caller-supplied
 * operands.  They work on any handle, touch no stream state and read nothing of the handle but its device, its row limit and its
 * poison knob; the packed output lives in scratch of the call and is returned row-major.  All synchronise `stream`.
 *
 * mmi_lm_debug_dep_attn: micro-step k of a frame, for `rows` rows (model rows of a step, or the rows of a scoring pass).
 *   qkv       device bf16 [rows][3 * H * Dh]: the in_proj output (q, then k, then v); 16-byte aligned
 *   k_cache, v_cache   device bf16 [rows][H][steps][Dh], read (positions < k) and written (position k) in place; 16-byte aligned
 *   kernel    MMI_DEP_ATTN_AUTO = the step's own choice; or MMI_DEP_ATTN_8 (k_dep_attn8<4>), MMI_DEP_ATTN_ROWS16 (k_dep_attn<16>),
 *             MMI_DEP_ATTN_ROWS32 (k_dep_attn<32>) forced
 *   out       device bf16 [rows][H * Dh];  kernel_run (host, may be NULL): the kernel that was launched
 * Refuses: a null pointer, an unknown kernel (MMI_ERR_INVALID); Dh outside 1..64 (MMI_ERR_UNSUPPORTED); steps outside 1..32, k
 * outside [0, steps), H outside 1..1024, rows outside 1..max(128, the handle's max_batch) (MMI_ERR_SHAPE); a forced kernel that does
 * not admit the shape - MMI_DEP_ATTN_8 needs Dh % 8 == 0 and steps <= 8, MMI_DEP_ATTN_ROWS16 steps <= 16 - and misaligned operands
 * (MMI_ERR_UNSUPPORTED).
 *
 * mmi_lm_debug_dep_attn_out_proj: x + out_proj(attention) of ONE row with the packed out_proj weight of the handle's own depth layer
 * `layer`, micro-step k in [1, dep_q); H, Dh and steps are the handle's (depformer_num_heads, depformer_dim / heads, dep_q).
 *   qkv [3 * dd], k_cache / v_cache [H][dep_q][Dh] (in place), x [dd] the residual row, out [dd]: device bf16, dd = depformer_dim
 *   fused     != 0: k_dep_attn_out_proj with the step's plan; 0: the two launches it replaces - launch_dep_attn, then the out_proj
 *             GEMM through the step's launch_gemm - and att (device bf16 [dd], may be NULL) also receives the attention output
 *   kernel_run (host, may be NULL): MMI_DEP_ATTN_FUSED, or the attention kernel of the two-launch form
 * Refused (MMI_ERR_UNSUPPORTED) where the step would not run this out_proj with the attention inside (more than one row is not
 * offered; int8 / fp8 / MXFP4 weights, an adapter handle, MMI_NO_DEP_ATTN_FUSION, head dims and steps k_dep_attn8 does not take,
 * a K split that is no whole heads).
 *
 * mmi_lm_debug_cross_attn: k_lm_cross_attn.
 *   q         device bf16 [rows][H * Dh];  kv device bf16 [rows][cap][2 * H * Dh] (keys, then values); both 16-byte aligned
 *   len       device int32 [rows]: live positions per row; every len in [1, cap] (checked on the host: MMI_ERR_INVALID)
 *   Dh        32, 64 or 128;  rows 1..max(128, the handle's max_batch);  cap 1..2^20
 *   out       device bf16 [rows][H * Dh] */
enum { MMI_DEP_ATTN_AUTO = 0, MMI_DEP_ATTN_8 = 1, MMI_DEP_ATTN_ROWS16 = 2, MMI_DEP_ATTN_ROWS32 = 3, MMI_DEP_ATTN_FUSED = 4 };
int mmi_lm_debug_dep_attn(mmi_lm* lm, const void* qkv_bf16, void* k_cache, void* v_cache, int32_t rows, int32_t H, int32_t Dh,
                          int32_t steps, int32_t k, int32_t kernel, void* out_bf16, int32_t* kernel_run, mmi_stream stream);
int mmi_lm_debug_dep_attn_out_proj(mmi_lm* lm, int32_t layer, int32_t k, int32_t fused, const void* qkv_bf16, void* k_cache,
                                   void* v_cache, const void* x_bf16, void* out_bf16, void* att_bf16, int32_t* kernel_run,
                                   mmi_stream stream);
int mmi_lm_debug_cross_attn(mmi_lm* lm, const void* q_bf16, const void* kv_bf16, const int32_t* len, int32_t rows, int32_t H,
                            int32_t Dh, int32_t cap, void* out_bf16, mmi_stream stream);

/* ---- chunked prefill of known frames into a live session (no reference counterpart) ----------------------------
 * mmi_lm_prefill on sessions S with T frames equals T calls of mmi_lm_step under an exec mask that holds exactly the sessions of S,
 * each preceded by mmi_lm_force_next_tokens with every entry of those sessions' rows >= 0, the previous exec mask restored
 * afterwards - except that
 *   1. no logits, no tokens and no output frame are produced: the text head, the depth transformer, the samplers and the extra
 *      heads do not run;
 *   2. the handle-wide draw counter does not advance and the depth transformer's per-frame cache is not touched: what a neighbour
 *      samples does not depend on whether a session was prefilled between two steps;
 *   3. the temporal K/V rings of layers >= 1 may differ from the stepped ones by attention summation order; everything else in the
 *      streaming state of the named sessions is what stepping leaves, bit for bit (offsets, the token delay ring, the text history
 *      of rows with sampling settings of their own, the last stored tokens);
 *   4. sessions not in S are untouched, byte for byte.
 * 128 known frames of one session cost one pass over the temporal weights instead of 128.
 *
 * mmi_lm_enable_prefill(lm, rows): before streaming_start, like mmi_lm_enable_nucleus.  rows = the row budget of one pass, 1..128
 * (0 = off again); the next streaming_start allocates the scratch of a pass beside - not inside - the streaming-state arena:
 * mmi_lm_state_bytes and snapshots are unchanged, and a handle that never enables it allocates nothing, launches nothing new and
 * runs the device code it ran before.  Refused with MMI_ERR_UNSUPPORTED (the message names the reason; nothing is written):
 * rows > 128; rows > 32 on a handle whose weights are packed at the 16-row tile (max_batch <= 16); quantised linears (int8, fp8,
 * MXFP4); cross-attention layers; an adapter handle; a handle with the TTS machine enabled; a head dim other than 32 / 64 / 128.
 * (A guided stream and per-step hooks are properties of a stream, not of the handle: mmi_lm_prefill refuses those, below; adapters or
 * the TTS machine enabled after this call are refused by the next streaming_start.)  MMI_ERR_STATE while streaming.
 *
 * mmi_lm_prefill(lm, sessions, n, user_codes, tokens, T, stream): stream ordered, no synchronisation.
 *   sessions    HOST int32 [n]: distinct indices in [0, streaming batch); 1 <= n <= rows.  They may stand at any offsets, and at
 *               different ones; continuing a live session is allowed
 *   user_codes  device i64 [n][n_q - dep_q][T]: what mmi_lm_step takes, per frame (NULL where the model has no user stream)
 *   tokens      device i64 [n][1 + dep_q][T]: what mmi_lm_force_next_tokens takes, per frame; every entry >= 0
 *   T           >= 1; cut into passes of floor(rows / n) frames.  A pass may straddle the ring's wrap and T may exceed the context
 * MMI_ERR_STATE: not streaming, or prefill not enabled.  MMI_ERR_INVALID: a session out of range or named twice, T < 1, more
 * sessions than rows.  MMI_ERR_UNSUPPORTED: a guided stream, or per-step hooks installed.
 * The host's step counter (what mmi_lm_step's `valid` is derived from, lm.py:774-776) advances by T, as T masked steps would
 * advance it - also when only some sessions were named: the next mmi_lm_step may then report valid = 1 for a stream whose other
 * sessions are younger than max_delay (their rows hold -2, as under support_out_of_sync).
 *
 * mmi_lm_last_tokens: a copy of the tokens the last step (or prefill) stored, device i64 [streaming batch][1 + dep_q] in step
 * coordinates (text, then the audio codebooks) - the log a caller keeps to hand a session back to mmi_lm_prefill; mmi_lm_step's
 * own return value lags by up to max_delay frames.  Stream ordered. */
int mmi_lm_enable_prefill(mmi_lm* lm, int32_t rows);
int32_t mmi_lm_prefill_rows(const mmi_lm* lm);          /* 0 = off; a negative status for a NULL handle */
int mmi_lm_prefill(mmi_lm* lm, const int32_t* sessions, int32_t n, const int64_t* user_codes, const int64_t* tokens, int32_t T,
                   mmi_stream stream);
int mmi_lm_last_tokens(mmi_lm* lm, int64_t* out, mmi_stream stream);

/* Parity tap of the prefill attention (tests): k_lm_attn_prefill alone, launched through the function the prefill pass uses, on
 * caller-supplied operands.  Works on any handle and touches no stream state.
 *   q          device bf16 [rows][H][Dh], taken as already roped
 *   row_ring   device int32 [rows], row_pos device int64 [rows]: the row table of a pass - n_blocks equal blocks of rows / n_blocks
 *              rows; the rows of a block name ONE ring in [0, rings) and consecutive positions from a start >= 0
 *   k_ring, v_ring     the layout of mmi_lm_debug_kv_ring for `rings` rings of `cap` slots: positions below a block's start, as a
 *              stream that stands at that start holds them
 *   k_staged, v_staged the block itself in ring format: [rows][H][row bytes], then (4-bit) the scale bytes [rows][H][Dh / 16]
 *   out        device bf16 [rows][H * Dh]
 * Row r attends position pos iff 0 <= row_pos[r] - pos < context.  rows <= 128.  Synchronises `stream`. */
int mmi_lm_debug_prefill_attn(mmi_lm* lm, const void* q_bf16, const int32_t* row_ring, const int64_t* row_pos, const void* k_ring,
                              const void* v_ring, const void* k_staged, const void* v_staged, int32_t rows, int32_t n_blocks,
                              int32_t rings, int32_t H, int32_t Dh, int32_t cap, int32_t context, int32_t kv_dtype, void* out_bf16,
                              mmi_stream stream);

/* ---- teacher-forced scoring of known frames on the prefill path ------------------------------------------------
 * The counterpart of LMModel.forward (lm.py:322-377: the text head over all positions, and forward_depformer_training, lm.py:410-448,
 * the depth transformer over all positions with the given tokens as its inputs), on a live session.
 *
 * mmi_lm_score on sessions S with T frames is the sequence of T forced steps that defines mmi_lm_prefill (exec mask = S, every
 * step preceded by mmi_lm_force_next_tokens with every entry >= 0) and returns, for every (session, frame, site) - site 0 the text
 * head, sites 1 .. dep_q the audio heads - what that step's parity taps return; under forcing micro-step k's input is the given
 * token of site k - 1 of the same frame.  These are raw model logits: temperature, repetition penalty, top-k, top-p and
 * per-session sampling settings play no part.  128 known frames cost one pass over the weights instead of 128 steps.
 *
 * mmi_lm_enable_score(lm, on): after mmi_lm_enable_prefill, before streaming_start.  The next streaming_start allocates the scoring
 * scratch beside the prefill scratch, outside the streaming-state arena: mmi_lm_state_bytes and snapshots are unchanged, and a
 * handle with prefill but without scoring allocates and launches what it did.  MMI_ERR_STATE while streaming or without prefill;
 * MMI_ERR_UNSUPPORTED (by name) for low-rank or demuxed depformer embeddings, for more than 32 rows per pass with the depth
 * transformer on its own 16-row tile, and for a head whose width is no multiple of 8 or exceeds 32768.
 *
 * mmi_lm_score(lm, sessions, n, user_codes, tokens, T, commit, out, stream): arguments as mmi_lm_prefill.  Stream ordered, nothing
 * synchronises.
 *   commit = 1  the named sessions end exactly where mmi_lm_prefill of the same arguments leaves them - every region of the state
 *               arena, all rings included, byte for byte (the same kernels in the same order).  T may span several passes.
 *   commit = 0  nothing of the handle's streaming state changes (no offsets, no rings, no delay ring): pure rescoring.  The call
 *               must fit one pass: n * T > rows is refused with MMI_ERR_INVALID.
 *   In both modes sessions not named are untouched, and neither the draw counter nor the step's depth-transformer cache is
 *   written: what a neighbour samples does not depend on a score call between two steps.
 *   out->logp          device f32 [n][T][1 + dep_q]: ln softmax(logits)[given token], in fp32 from the bf16 head output; -inf where
 *                      the given token lies outside the head's range (an initial-token id).  Must not be NULL
 *   out->argmax        device i32 [n][T][1 + dep_q] or NULL: the lowest index among the largest logits
 *   out->text_logits   device f32 [n][T][text_card_out] or NULL
 *   out->audio_logits  device f32 [n][T][dep_q][card] or NULL
 *   A NaN logit makes that site's logp NaN (its argmax is then unspecified).
 * Refusals, all before anything is written: every refusal of mmi_lm_prefill in its own words; MMI_ERR_STATE when scoring is not
 * enabled; MMI_ERR_INVALID for a NULL out or out->logp and for commit = 0 beyond one pass.
 *
 * mmi_lm_debug_score_rows: parity tap of the output kernel (tests) - k_score_logprob alone, through the pass's launch function, on
 * caller-supplied rows: logits_bf16 device bf16 [rows][N] (16-byte aligned, N a multiple of 8, <= 32768), targets device i32
 * [rows], logp f32 [rows], argmax i32 [rows], logits_f32 f32 [rows][N] or NULL.  Any handle; touches no stream state. */
struct mmi_score_out {
    float* logp;
    int32_t* argmax;
    float* text_logits;
    float* audio_logits;
};
typedef struct mmi_score_out mmi_score_out;
int mmi_lm_enable_score(mmi_lm* lm, int32_t on);
int32_t mmi_lm_score_enabled(const mmi_lm* lm);         /* a negative status for a NULL handle */
int mmi_lm_score(mmi_lm* lm, const int32_t* sessions, int32_t n, const int64_t* user_codes, const int64_t* tokens, int32_t T,
                 int32_t commit, const mmi_score_out* out, mmi_stream stream);
int mmi_lm_debug_score_rows(mmi_lm* lm, const void* logits_bf16, const int32_t* targets, int32_t rows, int32_t N, float* logp,
                            int32_t* argmax, float* logits_f32, mmi_stream stream);

/* ---- log-probabilities of the stored tokens and top-N alternatives in the live step -----------------------------
 * mmi_lm_enable_logprobs(lm, on, top_n): before streaming_start; top_n in 0..8 alternatives per site.  The stream then runs ONE
 * more launch per step, k_step_logprob in front of the ring commit (site label "logprob"), on every handle the step works on:
 * quantised linears and rings, guided streams, cross-attention, adapters, the TTS machine, hooks, the nucleus samplers.  It samples
 * the tokens it sampled.  The results live in float rings beside the streaming-state arena: mmi_lm_state_bytes and snapshots are
 * what they were; a handle without the option allocates and launches what it did.
 *
 * Per (session, site) - site 0 the text head, sites 1 .. dep_q the audio heads:
 *   logp      ln softmax(logits)[token] in fp32 on the bf16 logits as they stand when the step commits (after the guidance mix and
 *             the sampler's written-back padding bonus: what the step's parity taps return), for the token mmi_lm_last_tokens
 *             returns - after forcing and after the hooks; under the TTS machine the SAMPLED audio token, even where the audio
 *             rule stores another one.  -inf where the token lies outside the head's range (a forced initial-token id).
 *             Temperature, penalties, top-k and top-p play no part.  The arithmetic is mmi_lm_score's, bit for bit.
 *   top_id    the top_n entries first in the order (logit descending, index ascending); top_logp their log-probabilities.
 *   A NaN logit makes logp NaN (the alternatives are then unspecified).
 * Two stream-ordered read-outs (no synchronisation), valid until the next step, reset or seek; device outputs logp f32 [G][S],
 * top_id i32 / top_logp f32 [G][S][top_n] (both or neither; S = 1 + dep_q):
 *   mmi_lm_last_logprobs   step coordinates: lines up with mmi_lm_last_tokens.  A row that did not execute keeps its last executed
 *                          step's values; one that has not executed since the start or its reset reads NaN / id -1.
 *   mmi_lm_frame_logprobs  frame coordinates: lines up with the frame the last mmi_lm_step returned - NaN / -1 exactly where that
 *                          frame holds -2, and elsewhere the values recorded when the frame's token was sampled.
 * mmi_lm_reset, mmi_lm_state_load, mmi_lm_seek, mmi_lm_prefill and a committing mmi_lm_score return the rows they name to NaN / -1.
 * Refusals, before anything is written: MMI_ERR_INVALID for top_n outside 0..8, a NULL logp, or top_* on a handle with top_n == 0;
 * MMI_ERR_STATE for enabling while streaming and for a read-out on a handle without the option or not streaming.
 *
 * mmi_lm_debug_step_logprob: parity tap (tests) - k_step_logprob through the step op's launch function on caller rows: logits_bf16
 * device bf16 [rows][N], targets device i32 [rows], logp f32 [rows], top_id / top_logp [rows][top_n] or NULL.  MMI_ERR_UNSUPPORTED
 * for N % 8 != 0, N > 32768 or logits that are not 16-byte aligned.  Any handle; touches no stream state; synchronises. */
int mmi_lm_enable_logprobs(mmi_lm* lm, int32_t on, int32_t top_n);
int mmi_lm_logprobs_enabled(const mmi_lm* lm, int32_t* top_n_or_null);      /* 0 / 1; a negative status for a NULL handle */
int mmi_lm_last_logprobs(mmi_lm* lm, float* logp, int32_t* top_id, float* top_logp, mmi_stream stream);
int mmi_lm_frame_logprobs(mmi_lm* lm, float* logp, int32_t* top_id, float* top_logp, mmi_stream stream);
int mmi_lm_debug_step_logprob(mmi_lm* lm, const void* logits_bf16, const int32_t* targets, int32_t rows, int32_t N, int32_t top_n,
                              float* logp, int32_t* top_id, float* top_logp, mmi_stream stream);

/* The regions of the streaming-state arena - the buffer of mmi_lm_state_save - by name (tests compare two streams region by
 * region): one line "name<TAB>offset<TAB>bytes<TAB>rows<TAB>kind" each.  rows > 0: the region is `rows` equal slices, one per
 * session (model row); kind 1 = state the next step reads ("exec", "offsets", "cache", "text_tok", "audio_tok", "rng", "rowtab",
 * "thist", "coefs", "cond", and the temporal rings layer by layer: "kc.<l>", "vc.<l>", a 4-bit ring's "kc.<l>.scale"), kind 0 =
 * scratch that every step rewrites before reading it.  Returns the bytes needed including the final NUL (buf = NULL to size); 0
 * when not streaming. */
int64_t mmi_lm_debug_state_regions(const mmi_lm* lm, char* buf, int64_t cap);

/* The launch list of one frame step, recorded while the step ran for the first time: one line "site<TAB>kernel[<TAB>weight bytes]" per kernel
 * launch in launch order (sites: "L.in_proj", "L.ffn_in", "dep.out_proj", "text_linear", ...).  scripts/rocpd_sites.py joins
 * it with a rocprofv3 kernel trace by position inside the step, which is how per-site durations of kernels that share one
 * name are recomputed under profiles/.  Returns the bytes needed including the final NUL (call with buf = NULL to size);
 * 0 before the first step.  mmi_mimi_launch_list: which = 0 encoder step, 1 decoder step. */
int64_t mmi_lm_launch_list(const mmi_lm* lm, char* buf, int64_t cap);
int64_t mmi_mimi_launch_list(const mmi_mimi* m, int32_t which, char* buf, int64_t cap);

/* Test / benchmark aid (no reference counterpart): move every session to stream position offsets[b] (host i64 [batch]) WITHOUT
 * touching the KV ring - the positions skipped read whatever the ring holds (zeros after streaming_start).  Lets the ring
 * wrap at the real capacity (context 3000) be exercised in seconds, and a full-context step be timed without 3000 warm-up
 * steps.  The host step counter becomes max(offsets). */
int mmi_lm_seek(mmi_lm* lm, const int64_t* offsets, mmi_stream stream);

/* Dominant-kernel timing tap for bench.py's roofline object: when enabled, steps run un-graphed and
 * every launch of the widest weight-streaming GEMM is bracketed by hipEvents on `stream`. */
int mmi_lm_profile_begin(mmi_lm* lm);
/* Per-site timings of the steps run since mmi_lm_profile_begin: one line "site<TAB>ops<TAB>total ms<TAB>weight bytes per op"
 * per site of the launch list (hipEvent pairs around every op of the un-graphed steps; dispatch gaps included).  Call before
 * mmi_lm_profile_end; synchronises the stream.  Returns the bytes needed including the final NUL (buf = NULL to size). */
int64_t mmi_lm_profile_sites(mmi_lm* lm, char* buf, int64_t cap);
/* Returns the mean duration (ms) and launch count since mmi_lm_profile_begin, plus the algorithmic
 * bytes one such launch streams (packed weight bytes + activations in/out). Synchronises the stream. */
int mmi_lm_profile_end(mmi_lm* lm, double* mean_ms, int64_t* n_launches, int64_t* bytes_per_launch,
                       const char** kernel_name);

/* Architecture the handle was created with (what callers read as attributes: frame_size, num_codebooks, dep_q ...). */
int mmi_mimi_get_cfg(const mmi_mimi* m, mmi_mimi_cfg* out);
int mmi_lm_get_cfg(const mmi_lm* lm, mmi_lm_cfg* out);

/* ------------------------------------------------------------------------------------------ */
/* Duplex pipeline: the frame step  encode -> LMGen.step -> decode  software-pipelined        */
/* ------------------------------------------------------------------------------------------ */
/* The reference's serving loop runs the three calls of a frame back to back on one stream (server.py:132-146).  Their
 * streaming states are disjoint: encode(t+1) depends on encode(t) only, decode(t) on LMGen.step(t) and decode(t-1).  A duplex
 * pipeline owns three HIP streams (encoder, LM, decoder) and the events between them, so that - when frames are submitted
 * back to back (offline inference, several session groups per GPU, a loaded server) - encode(t+1) and decode(t-1) run in the
 * shadow of LMGen.step(t), whose depth-transformer phase leaves most CUs idle.  Results are bit-identical to the serial
 * schedule (same kernels, same per-stream order).  The DEVICE is never synchronised, but the HOST is: mmi_duplex_submit(t)
 * blocks the calling thread (hipEventSynchronize) until LMGen.step(t-2) has completed (flow control: two steps in flight at
 * most) and until LMGen.step(t-1) has reached its depth-transformer phase (the gate behind which the codec work of frame t is
 * enqueued, csrc/duplex.hip) - in steady state it returns about one LM temporal phase after it was called.
 *
 *   mmi_duplex_submit   frame t: pcm_in f32 [batch, 1, frame_size] -> pcm_out f32 [batch, 1, frame_size] (written when the
 *                       frame's decode ran; untouched while *valid == 0, i.e. where LMGen.step returns None) and, optionally,
 *                       tokens_out i64 [batch, 1 + dep_q, 1] (LMGen.step's output, -2 rows included).  Work submitted on
 *                       `caller` before the call is ordered before the frame (inputs, set_exec_mask / reset_streaming issued
 *                       on the handles with that stream after a mmi_duplex_join).  At most two frames are in flight: the call
 *                       blocks the host until frame t-2 has completed.  pcm_in is copied into the pipeline's own input ring in
 *                       `caller`'s stream order: the caller may refill it as soon as the call returns (as after
 *                       MimiModel.encode).  pcm_out / tokens_out stay unread until a mmi_duplex_join on the consuming stream.
 *                       `batch` must equal the streaming batch (MMI_ERR_SHAPE otherwise, like mmi_lm_step).
 *                       MMI_ERR_UNSUPPORTED while the LM has per-step hooks installed (mmi_lm_set_hooks): the hooks work on the
 *                       caller's stream, the pipeline steps the LM on its own - a hooked LMGen goes through mmi_lm_step.
 *   mmi_duplex_join     makes `caller` wait (device side) for every frame submitted so far.
 * Both handles must be streaming with the same batch before mmi_duplex_create and must not be driven through their own
 * step entry points between a submit and the next join.  A call that fails half-way (a launch error inside a frame) leaves the
 * three stream orders inconsistent: the pipeline is dead from then on - submit / join / flush return MMI_ERR_STATE, waiters are
 * released - and must be destroyed. */
typedef struct mmi_duplex mmi_duplex;
int mmi_duplex_create(mmi_mimi* mimi, mmi_lm* lm, mmi_duplex** out);
void mmi_duplex_destroy(mmi_duplex* d);
int mmi_duplex_submit(mmi_duplex* d, const float* pcm_in, float* pcm_out, int64_t* tokens_out_or_null, int32_t batch,
                      int32_t* valid, mmi_stream caller);
int32_t mmi_duplex_batch(const mmi_duplex* d);      /* the streaming batch the pipeline was created with */
int mmi_duplex_join(mmi_duplex* d, mmi_stream caller);
/* The host-side form: blocks the calling thread until every submitted frame has completed (its outputs are then readable from any
 * stream).  Unlike mmi_duplex_join it leaves no waiter on the device while the frames run. */
int mmi_duplex_flush(mmi_duplex* d);
/* Diagnostics: with the timeline on, every submit records timestamps around the frame's three phases on their streams;
 * mmi_duplex_get_timeline synchronises the pipeline and returns ms since the LAST submit reached the caller's stream:
 * {encode begin, encode end, LM begin, -, LM end, decode begin, decode end} (host f32[7]); entries of phases that did not run
 * are -1.  One set of events serves every frame, so the seven entries belong to ONE frame only when a mmi_duplex_flush follows
 * every submit (one frame alone in the pipeline: what bench.py's p50 / p95 measure); with frames in flight the decode entries are
 * those of frame t-2.  Per-frame figures in steady state: mmi_duplex_get_stamps. */
int mmi_duplex_set_timeline(mmi_duplex* d, int32_t on);
int mmi_duplex_get_timeline(mmi_duplex* d, float* ms7);
/* Diagnostics, finer: with the timeline on the pipeline also stamps the device's constant-rate clock at its hand-off points
 * (one-thread kernels on the three streams).  Returns ms40[4][10] - frames t & 3 of the last four submits; per frame: input
 * published, encode begin / end, the LM's wait for the encoder begin / end, LM begin, depth-transformer phase, LM end, decode
 * begin / end - in ms since the oldest stamp held (-1: not stamped; the clock's rate is hipDeviceAttributeWallClockRate), and the
 * number of the last submitted frame. */
int mmi_duplex_get_stamps(mmi_duplex* d, double* ms40, int64_t* last_frame);

/* ------------------------------------------------------------------------------------------ */
/* Session batcher: many live dialogue sessions on one GPU                                    */
/* ------------------------------------------------------------------------------------------ */
/* SURVEY.md 8f-1.  The reference's Python server runs ONE session under a lock (server.py:45,57,154-169);
 * its Rust server packs up to `batch_size` live channels into one batched model step with a per-row stream
 * mask and a per-row reset when a channel is (re)opened (rust/moshi-server/src/batched_asr.rs:188-276 model
 * loop, :279-374 pre_process, :376-437 post_process; py_module.rs:443-470 slot allocation).  This is that
 * model loop for the full-duplex path, on top of the entry points above:
 *
 *   every mmi_batcher_step:  per slot, take one 80 ms frame from the channel's PCM FIFO if it holds one (exec mask),
 *   reset the rows of channels opened since the last step, then  Mimi encode -> LMGen.step -> Mimi decode  on the
 *   whole batch, and hand each executed row's (text token, audio tokens, PCM frame) to its channel's output FIFO.
 *
 * Host pointers here are HOST memory: the batcher owns pinned staging buffers and its own HIP stream.
 * open/close/push/pop may be called from any thread; step from one thread at a time (the model loop). */
typedef struct mmi_batcher_cfg {
    int32_t slots;                          /* rows of the batch = concurrent channels; <= both handles' max_batch */
    int32_t reset_codec_after_first_frame;  /* server.py:135-141: the first input frame's encoder state is dropped  */
    int32_t max_buffered_frames;            /* per-channel cap on queued input frames and on un-popped output frames */
    mmi_sampling sampling;                  /* LMGen constructor arguments (lm.py:557-574)                          */
    mmi_guidance guidance;                  /* cfg_coef = 0 or 1: none.  Otherwise as mmi_lm_streaming_start_guided: what every
                                               channel gets that does not bring its own (mmi_batcher_open_cond; server.py:53-54:
                                               one condition for the model type); the LM handle then needs max_batch >= 2 * slots */
} mmi_batcher_cfg;

typedef struct mmi_batcher_stats {
    int64_t steps;            /* model steps run (iterations that had at least one row with data)          */
    int64_t frames;           /* session-frames executed (sum of active rows over steps)                   */
    int64_t dropped_frames;   /* output frames dropped because a channel's output FIFO was full            */
    int32_t used_slots, total_slots;
    float last_step_ms;       /* device time of the last step (hipEvents on the batcher's stream)          */
} mmi_batcher_stats;

typedef struct mmi_batcher mmi_batcher;

/* Puts both models into streaming mode with batch = cfg->slots (streaming_forever, server.py:59-60).  The handles must
 * outlive the batcher and must not be driven by anyone else meanwhile. */
int mmi_batcher_create(mmi_mimi* mimi, mmi_lm* lm, const mmi_batcher_cfg* cfg, mmi_batcher** out);
void mmi_batcher_destroy(mmi_batcher* b);
/* Claim a free slot (py_module.rs:443-470); MMI_ERR_BUSY when all are taken.  The row's streaming state is reset at
 * the next step (handle_chat: mimi.reset_streaming(); lm_gen.reset_streaming(), server.py:163-164). */
int mmi_batcher_open(mmi_batcher* b, int64_t* channel_id);
/* The same with the channel's own sampling settings (stream_both.rs:95-105): the slot's row gets them, with its reset, before
 * its first step.  NULL = mmi_batcher_open: the batcher's cfg.sampling (also for a slot whose last owner had settings).
 * Settings mmi_row_sampling_check refuses are refused here, and no slot is claimed. */
int mmi_batcher_open_with(mmi_batcher* b, const mmi_row_sampling* settings_or_null, int64_t* channel_id);
/* A channel's own condition (tts.rs:342-357: voice and guidance strength per request).  HOST memory, like everything else at
 * this boundary; the fields are those of mmi_row_condition. */
struct mmi_batcher_condition {
    float cfg_coef;
    const void* condition_sum;           /* host bf16 [R, dim] or NULL; R = 1, or 2 when the batcher runs guided */
    const void* condition_cross;         /* host bf16 [R, cross_len, dim] or NULL */
    int32_t cross_len;
};
typedef struct mmi_batcher_condition mmi_batcher_condition;
/* mmi_batcher_open_with plus the channel's own condition.  The arrays are copied at once (the caller's may go away); at the next
 * step the slot's rows get them (one host-to-device copy, then mmi_lm_set_row_condition on the batcher's stream) with the slot's
 * reset, before the row's first step.  cond_or_null == NULL: the batcher's own cfg.guidance rows of that slot, also for a slot
 * whose last owner had a condition (the batcher keeps a copy of them).  Room for sources longer than cfg.guidance.cross_len
 * is a property of the LM handle: mmi_lm_set_cross_capacity before mmi_batcher_create.  A condition mmi_lm_set_row_condition
 * would refuse is refused here with the same status, and no slot is claimed. */
int mmi_batcher_open_cond(mmi_batcher* b, const mmi_row_sampling* settings_or_null, const mmi_batcher_condition* cond_or_null,
                          int64_t* channel_id);
/* mmi_batcher_open_cond for a channel that runs on adapter slot `adapter_slot` (-1 = none) of an adapter handle
 * (mmi_lm_enable_adapters before mmi_batcher_create): the slot's row gets it with the slot's reset, before the row's first step,
 * and keeps it for the channel's life; mmi_batcher_close returns the row to -1.  A slot mmi_lm_set_row_adapter would refuse is
 * refused here with the same status, and no slot is claimed. */
int mmi_batcher_open_lora(mmi_batcher* b, const mmi_row_sampling* settings_or_null, const mmi_batcher_condition* cond_or_null,
                          int32_t adapter_slot, int64_t* channel_id);
/* The channel's row samples with its own (top_p, top_p_text) from the next step on, for the channel's life (a batcher on a handle
 * with mmi_lm_enable_nucleus before mmi_batcher_create); the row returns to the handle's values at the step after the close, as an
 * adapter slot does.  What mmi_lm_set_row_top_p would refuse is refused here with the same status. */
int mmi_batcher_set_channel_top_p(mmi_batcher* b, int64_t channel_id, float top_p, float top_p_text);
/* A new channel that continues from `parent_channel`'s state (no reference counterpart: batched_asr.rs opens every slot fresh;
 * the nearest is get_streaming_state / set_streaming_state on a batch of one, streaming.py:158-181).  Claims a free slot
 * (MMI_ERR_BUSY: none; MMI_ERR_NO_CHANNEL: unknown parent; MMI_ERR_STATE: the parent was opened since the last step and has no
 * state yet) and runs mmi_mimi_fork_session and mmi_lm_fork_session on the batcher's stream, behind the last step and in front
 * of the next.  The child takes the parent's bookkeeping (own sampling, condition, adapter, top_p, frame counter), starts with
 * empty input and output FIFOs and is not reset at its first step; settings_or_null != NULL: its row then gets those settings
 * (mmi_lm_set_row_sampling) - a seed of its own makes it a different candidate.  Closing the parent later leaves the child. */
int mmi_batcher_fork(mmi_batcher* b, int64_t parent_channel, const mmi_row_sampling* settings_or_null, int64_t* channel_id);
int mmi_batcher_close(mmi_batcher* b, int64_t channel_id);
/* Append 24 kHz mono PCM (host f32) to the channel's FIFO (batched_asr.rs:77-90 extend_data). */
int mmi_batcher_push_pcm(mmi_batcher* b, int64_t channel_id, const float* pcm, int32_t n_samples);
/* One iteration of the model loop.  n_active (host) = rows that had a frame; 0 means nothing was run. */
int mmi_batcher_step(mmi_batcher* b, int32_t* n_active);
/* Next un-popped output frame of a channel: pcm f32[frame_size], tokens i64[1 + dep_q] (text, audio...), got = 0/1.
 * With an ASR-style LM (dep_q = 0, the batched_asr.rs case proper) nothing is decoded: tokens = the text token, pcm is zeros.
 * Frames produced while the LM's delay ring was still filling (tokens -2, lm.py:781-782) are never queued, exactly
 * like the reference server skips `None` (server.py:144-146). */
int mmi_batcher_pop(mmi_batcher* b, int64_t channel_id, float* pcm, int64_t* tokens, int32_t* got);
/* mmi_batcher_pop with the frame's log-probabilities (an LM handle with mmi_lm_enable_logprobs; MMI_ERR_STATE without): host
 * logp f32 [1 + dep_q], top_id i32 / top_logp f32 [1 + dep_q][top_n] or NULL - mmi_lm_frame_logprobs of the step that produced the
 * frame.  mmi_batcher_pop drops them with the frame. */
int mmi_batcher_pop_logprobs(mmi_batcher* b, int64_t channel_id, float* pcm, int64_t* tokens, float* logp, int32_t* top_id,
                             float* top_logp, int32_t* got);
int mmi_batcher_get_stats(mmi_batcher* b, mmi_batcher_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* MOSHI_MI_H_ */
