// Moshi LM kernels for gfx950 (bf16 weights/activations, fp32 accumulate/norm/rope/softmax - the same rounding
// points as the reference's eager bf16 path: every nn.Linear output, norm output, rope output and residual add
// is rounded to bf16; transformer.py:45-58, rope.py:11-82, gating.py:13-22, lm.py:379-408,450-493).
//
// Data layout in HBM
//   linear weights  packed at load into MFMA A-fragment order, one contiguous 1 KiB fragment per
//                   (n-tile, k-step): TN=32 -> v_mfma_f32_32x32x16_bf16, lane l holds W[nt*32+(l&31)][ks*16+8*(l>>5)+e];
//                   TN=16 -> v_mfma_f32_16x16x32_bf16, lane l holds W[nt*16+(l&15)][ks*32+8*(l>>4)+e].
//                   A wave streams its K-slice of an n-tile as consecutive non-temporal 16-byte-per-lane loads.
//                   The SiLU-gated FFN's linear_in interleaves gate rows and value rows inside each tile so that
//                   the epilogue can form silu(g)*u without another pass (gating.py:19-20).
//   activations     between GEMMs: MFMA B-fragment order Xp[mt][ks][lane][8] (see "fragment-packed layouts" below), written
//                   by the producing epilogue; only q (for attention), the depformer's qkv and the logits are row-major.
//   KV ring         [layer][2][B][H][cap][Dh] bf16 (row = one position of one head: 256 contiguous bytes at Dh=128).
//   token ring      [B][17][max_delay+2] int32 (lm.py:605-613).
#pragma once
#include "mmi_common.h"
#include "mmi_fp4.h"

// ------------------------------------------------------------------------------------------------
// fragment-packed layouts
// ------------------------------------------------------------------------------------------------
// Every GEMM of the step is out[b][n] = sum_k x[b][k] * W[n][k] with a handful of batch rows (one to four tiles of T) and weights
// that are read exactly once per step, i.e. an HBM stream.  Both operands are kept in HBM in the order the MFMA
// wants them in registers, so that one wave instruction (16 bytes per lane) is one contiguous, fully coalesced
// 1 KiB read that feeds one MFMA without any shuffling:
//   T = 32 (v_mfma_f32_32x32x16_bf16, 17..128 rows)   : k-step = 16; lane l holds rows/cols (l & 31), k = 8*(l>>5)+e
//   T = 16 (v_mfma_f32_16x16x32_bf16, <= 16 sessions) : k-step = 32; lane l holds rows/cols (l & 15), k = 8*(l>>4)+e
//   weights     Wp[nt][ks][lane][e] = W[nt*T + (l & (T-1))][ks*KS + 8*(l / T) + e]            (zero padded)
//   activations Xp[mt][ks][lane][e] = x[mt*T + (l & (T-1))][ks*KS + 8*(l / T) + e]            (zero padded)
// A GEMM epilogue writes its result straight into the packed layout of the GEMM that consumes it.
MMI_HD long mmi_xp_index(int T, int b, int k, int ksteps) {
    const int sh = T == 32 ? 4 : 5;                 // log2(k-step)
    const int mt = b / T, bl = b - mt * T;
    const int ks = k >> sh, kq = (k >> 3) & ((1 << (sh - 3)) - 1), e = k & 7;
    return ((((long)mt * ksteps + ks) * 64) + kq * T + bl) * 8 + e;
}
static inline int mmi_kstep(int T) { return T == 32 ? 16 : 32; }

// gate_hidden == 0: plain [N][K] matrix.  gate_hidden == H: rows [0,H) are gates, [H,2H) values; tile nt carries
// gate rows nt*TN/2 .. and, in its second half, the matching value rows (so the epilogue forms silu(g)*u locally).
__global__ void k_pack_w_bf16(const uint16_t* __restrict__ W, uint16_t* __restrict__ P, int N, int K, int TN, int NT,
                              int KSTEPS, int gate_hidden) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)NT * KSTEPS * 512;
    if (idx >= total) return;
    int e = (int)(idx & 7);
    int lane = (int)((idx >> 3) & 63);
    long rest = idx >> 9;
    int ks = (int)(rest % KSTEPS);
    int nt = (int)(rest / KSTEPS);
    int i, kq, kstep;
    if (TN == 32) { i = lane & 31; kq = lane >> 5; kstep = 16; } else { i = lane & 15; kq = lane >> 4; kstep = 32; }
    int k = ks * kstep + 8 * kq + e;
    long row;
    bool valid;
    if (gate_hidden > 0) {
        int half = TN / 2;
        int r = nt * half + (i < half ? i : i - half);
        valid = r < gate_hidden;
        row = (i < half ? 0 : gate_hidden) + r;
    } else {
        row = (long)nt * TN + i;
        valid = row < N;
    }
    uint16_t v = 0;
    if (valid && k < K) v = W[row * K + k];
    P[idx] = v;
}

// One slot of an adapter bank (GemmArgs::lora_*): k_pack_w_bf16 of the [N][K] matrix W, scaled (bf16(scale * w): lora_B carries
// the adapter's scaling, exact for powers of two; lora_A takes 1), into k-steps [ks0, ks0 + KSTEPS) of a packed weight whose
// tiles hold KSTEPS_DST k-steps.  W == nullptr: the slot's entries are zeroed (unload).
__global__ void k_pack_lora_slot(const uint16_t* __restrict__ W, uint16_t* __restrict__ P, int N, int K, int TN, int NT, int KSTEPS,
                                 int gate_hidden, int KSTEPS_DST, int ks0, float scale) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)NT * KSTEPS * 512;
    if (idx >= total) return;
    int e = (int)(idx & 7);
    int lane = (int)((idx >> 3) & 63);
    long rest = idx >> 9;
    int ks = (int)(rest % KSTEPS);
    int nt = (int)(rest / KSTEPS);
    int i, kq, kstep;
    if (TN == 32) { i = lane & 31; kq = lane >> 5; kstep = 16; } else { i = lane & 15; kq = lane >> 4; kstep = 32; }
    int k = ks * kstep + 8 * kq + e;
    long row;
    bool valid;
    if (gate_hidden > 0) {
        int half = TN / 2;
        int r = nt * half + (i < half ? i : i - half);
        valid = r < gate_hidden;
        row = (i < half ? 0 : gate_hidden) + r;
    } else {
        row = (long)nt * TN + i;
        valid = row < N;
    }
    uint16_t v = 0;
    if (W && valid && k < K) v = mmi_f32_to_bf16(mmi_bf16_to_f32(W[row * K + k]) * scale);
    P[(((long)nt * KSTEPS_DST + ks0 + ks) * 64 + lane) * 8 + e] = v;
}

// *bad = 1 when bf16(scale * w) is not finite for some w (adapter tensors are checked before anything is written: a zero
// activation against an Inf weight is a NaN in rows that do not even use the slot)
__global__ void k_lora_check_finite(const uint16_t* __restrict__ W, long n, float scale, int* __restrict__ bad) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const uint16_t v = mmi_f32_to_bf16(mmi_bf16_to_f32(W[idx]) * scale);
    if ((v & 0x7f80u) == 0x7f80u) *bad = 1;
}

// int8 weights (bitsandbytes-style per-output-row absmax quantisation, utils/quantize.py:13-22: `weight` int8 CB +
// `weight_scb` fp32 row absmax; W ~= CB * SCB / 127).  Same tile order as the bf16 packing with TWO k-steps per 16-byte
// lane entry: Wq[nt][kp][lane][16], entries 0..7 = k-step 2kp, 8..15 = k-step 2kp+1 (zero padded to an even count).
// The GEMM widens the bytes to bf16 in registers (exact: |q| <= 127) and scales the fp32 accumulator by SCB/127.
__global__ void k_pack_w_i8(const int8_t* __restrict__ W, int8_t* __restrict__ P, int N, int K, int TN, int NT, int KP,
                            int gate_hidden) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)NT * KP * 1024;
    if (idx >= total) return;
    int e = (int)(idx & 15);
    int lane = (int)((idx >> 4) & 63);
    long rest = idx >> 10;
    int kp = (int)(rest % KP);
    int nt = (int)(rest / KP);
    int i, kq, kstep;
    if (TN == 32) { i = lane & 31; kq = lane >> 5; kstep = 16; } else { i = lane & 15; kq = lane >> 4; kstep = 32; }
    int k = (2 * kp + (e >> 3)) * kstep + 8 * kq + (e & 7);
    long row;
    bool valid;
    if (gate_hidden > 0) {
        int half = TN / 2;
        int r = nt * half + (i < half ? i : i - half);
        valid = r < gate_hidden;
        row = (i < half ? 0 : gate_hidden) + r;
    } else {
        row = (long)nt * TN + i;
        valid = row < N;
    }
    int8_t v = 0;
    if (valid && k < K) v = W[row * K + k];
    P[idx] = v;
}

// MXFP4 weights (OCP Microscaling: `weight` = E2M1 codes, two per byte [N][K / 2]; `weight_scale_e8m0` = one E8M0 byte per 32
// input features [N][K / 32]; mmi_fp4.h).  Same tile order again with FOUR k-steps per 16-byte lane entry: Wq[nt][ke][lane][16],
// word j of the entry = the lane's eight codes of k-step 4ke + j (zero padded to whole entries).  The scale bytes travel in
// the same order, Sq[nt][ke][lane][SB], one byte per MX block the lane's entry touches: SB = 2 at the 32-row tile (a k-step
// is 16 features: words 0, 1 share byte 0, words 2, 3 byte 1), SB = 4 at the 16-row tile (a k-step is one block).  The lanes of
// one row hold the same bytes: a lane fetches its entry's scales with one 2- or 4-byte load next to the 16-byte entry.
// Padding carries scale byte 127 (2^0) over zero codes.  One thread per code byte.
__global__ void k_pack_w_fp4(const uint8_t* __restrict__ W, const uint8_t* __restrict__ S, uint8_t* __restrict__ P,
                             uint8_t* __restrict__ PS, int N, int K, int TN, int NT, int KE, int gate_hidden) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)NT * KE * 1024;
    if (idx >= total) return;
    int e = (int)(idx & 15);
    int lane = (int)((idx >> 4) & 63);
    long rest = idx >> 10;
    int ke = (int)(rest % KE);
    int nt = (int)(rest / KE);
    int i, kq, kstep;
    if (TN == 32) { i = lane & 31; kq = lane >> 5; kstep = 16; } else { i = lane & 15; kq = lane >> 4; kstep = 32; }
    int k = (4 * ke + (e >> 2)) * kstep + 8 * kq + 2 * (e & 3);      // the byte's low-nibble element; k + 1 sits in the high nibble
    long row;
    bool valid;
    if (gate_hidden > 0) {
        int half = TN / 2;
        int r = nt * half + (i < half ? i : i - half);
        valid = r < gate_hidden;
        row = (i < half ? 0 : gate_hidden) + r;
    } else {
        row = (long)nt * TN + i;
        valid = row < N;
    }
    uint8_t v = 0;
    if (valid && k < K) v = W[row * (K / 2) + (k >> 1)];
    P[idx] = v;
    const int SB = TN == 32 ? 2 : 4;
    if (e < SB) {
        const int blk = TN == 32 ? 2 * ke + e : 4 * ke + e;           // MX block (32 features) of the row
        uint8_t sc = 127;
        if (valid && blk * 32 < K) sc = S[row * (K / 32) + blk];
        PS[((rest * 64) + lane) * SB + e] = sc;
    }
}

// 16 int8 -> two bf16 fragments (k-step 2kp, k-step 2kp+1)
__device__ __forceinline__ void mmi_i8x16_to_bf16(u32x4 q, u32x4& lo, u32x4& hi) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t w = q[d];          // byte k sign-extended: shift it to the top as unsigned, arithmetic shift back down
        const float f0 = (float)((int)(w << 24) >> 24), f1 = (float)((int)(w << 16) >> 24), f2 = (float)((int)(w << 8) >> 24), f3 = (float)((int)w >> 24);
        const uint32_t p0 = mmi_pack_bf16x2(f0, f1), p1 = mmi_pack_bf16x2(f2, f3);
        if (d < 2) { lo[2 * d] = p0; lo[2 * d + 1] = p1; }
        else { hi[2 * (d - 2)] = p0; hi[2 * (d - 2) + 1] = p1; }
    }
}

// fp8 linears (BASELINE configs[4]: fp8 MFMA GEMMs): `weight` e4m3fn codes + `weight_scale` fp32 per output row (W ~= code *
// scale), packed exactly like the int8 bytes (two k-steps per 16-byte lane entry).  The activations stay bf16 in HBM and are
// converted to e4m3 in registers on their way into v_mfma_f32_{32x32x16,16x16x32}_fp8_fp8: x8 = e4m3(x / input_scale) with a
// static per-linear `input_scale` (a calibration constant, default 1), and the fp32 accumulator is scaled by
// weight_scale[row] * input_scale in the epilogue (folded into one per-row factor at load).
// 8 bf16 (one activation fragment) -> 8 fp8 bytes
__device__ __forceinline__ u32x2 mmi_bf16x8_to_fp8(u32x4 x, float inv) {
    float f[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f[2 * q] = __builtin_bit_cast(float, x[q] << 16) * inv;
        f[2 * q + 1] = __builtin_bit_cast(float, x[q] & 0xffff0000u) * inv;
    }
    u32x2 r;
    r[0] = mmi_cvt_fp8x4(f[0], f[1], f[2], f[3]);
    r[1] = mmi_cvt_fp8x4(f[4], f[5], f[6], f[7]);
    return r;
}

// ---- int8 activations (bitsandbytes int8_vectorwise_quant, utils/quantize.py:24-40; restated in oracle/lm_oracle.py) ----------
// max |v| over 8 packed bf16 values
__device__ __forceinline__ float mmi_absmax_bf16x8(u32x4 v) {
    float m = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        m = fmaxf(m, fabsf(__builtin_bit_cast(float, v[q] << 16)));
        m = fmaxf(m, fabsf(__builtin_bit_cast(float, v[q] & 0xffff0000u)));
    }
    return m;
}
// CA = int8(round_half_even(x * (127 / SCA))): 8 bf16 values -> 8 bytes (scale = 127 / SCA, 0 for an all-zero row).
// t = x * scale is rounded to fp32 like bitsandbytes' product, then t + 1.5 * 2^23 rounds it to the nearest integer, ties to
// even - the fp32 adder IS round-half-even at that magnitude, |t| <= 127 - and leaves the two's-complement byte in the low 8 bits
// of the sum: 3 instructions per element + a byte permute per pair instead of rint / convert / mask / shift / or (the
// quantisation sits on the dependent chain of the depth transformer's GEMMs, where every workgroup converts its own copy)
__device__ __forceinline__ u32x2 mmi_quant_i8x8(u32x4 v, float scale) {
    const float magic = 12582912.0f;            // 1.5 * 2^23
    u32x2 r;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned x0 = v[2 * h], x1 = v[2 * h + 1];
        const unsigned a = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, x0 << 16) * scale + magic);
        const unsigned b = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, x0 & 0xffff0000u) * scale + magic);
        const unsigned c = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, x1 << 16) * scale + magic);
        const unsigned d = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, x1 & 0xffff0000u) * scale + magic);
        r[h] = mmi_pack_low_bytes(a, b, c, d);
    }
    return r;
}
__device__ __forceinline__ float mmi_i8_scale(float sca) { return sca > 0.f ? 127.0f / sca : 0.f; }
// The dequantisation of oracle/lm_oracle.py `linear_int8` - a RESTATEMENT of bitsandbytes' int8_mm_dequant, `out32 * (row_stats *
// col_stats) * (1 / 127^2)` left to right in fp32, as its "default" backend writes it; not verified against the library, whose CUDA
// kernel multiplies by a literal constant and returns fp16 (PARITY UNPINNED).  The engine's int8 x int8 linears
// are bit-identical to THAT RESTATEMENT for the same bf16 input row (tests: *_int8_linear_bit_exact_*)
__device__ __forceinline__ float mmi_i8_dequant(int out32, float sca, float scb) {
    return ((float)out32 * (sca * scb)) * (1.0f / (127.0f * 127.0f));
}

// ------------------------------------------------------------------------------------------------
// weight-streaming skinny GEMM
// ------------------------------------------------------------------------------------------------
// grid.x = groups of NTW n-tiles; the block's WAVES waves split K (contiguous slices), each wave streams its slice of
// the NTW weight tiles with U fragments per tile in flight in each of two register buffers (explicit double
// buffering: the loads of group g+1 are issued before the MFMAs of group g), reading the matching activation
// fragments from L2.  The waves' partial tiles are summed through LDS in a fixed order (deterministic), and the
// epilogue (bf16 rounding point of nn.Linear, residual add, SiLU gate, embedding add) writes 8 consecutive features
// of one session as one 16-byte vector.
enum { MMI_EPI_STORE = 0, MMI_EPI_RESID = 1, MMI_EPI_GATE = 2, MMI_EPI_EMB = 3, MMI_EPI_PARTIAL = 4, MMI_EPI_ROPE_KV = 5, MMI_EPI_DEP_QKV0 = 6, MMI_EPI_LORA_T = 7 };
enum { MMI_OUT_ROWMAJOR = 0, MMI_OUT_PACKED = 1 };

struct GemmArgs {
    const u32x4* wp;        // packed weights [NT][KSTEPS][64]
    const u32x4* xp;        // packed activations [MT][KSTEPS][64]
    uint16_t* out;          // row-major [B][out_ld] or packed [.][out_ksteps][64][8]
    const uint16_t* resid;  // EPI_RESID: same geometry as out
    const uint16_t* emb;    // EPI_EMB: embedding table [rows][N]
    union {
    const int* tok;         // EPI_EMB: token per session, tok[(b % tok_rows) * tok_stride] (model rows beyond tok_rows are the
    const int* row_slot;    // MMI_EPI_LORA_T: adapter slot of session b % tok_rows (guidance twins follow their session), -1 = none
    };
    union {
    int tok_stride;         // guidance twins of the sessions and take the same token)
    int lora_rank;          // MMI_EPI_LORA_T: R, the columns of one slot (a multiple of 32: a task's 8 features share a slot)
    };
    int tok_rows;
    int B, N, KSTEPS, NT;
    int out_mode, out_ld, out_ksteps;
    int epi;
    const float* wscale;    // int8 / fp8 weights: dequantisation factor per ORIGINAL weight row (gate rows [0,H), value rows [H,2H)); else null
    const float* wscb;      // int8 weights: the raw row absmax SCB (`weight_scb`), read by the int8 x int8 dequantisation
                            // out32 * (SCA[b] * SCB[n]) * (1 / 127^2) - the oracle's restatement of bitsandbytes' int8_mm_dequant, in its order
    float xinv;             // fp8: 1 / input_scale, applied to the activations before the e4m3 conversion
    int wq;                 // host side only: 0 bf16, 1 int8 (widened to bf16), 2 fp8 (fp8 MFMA) weights, 3 int8 weights x int8 activations,
                            // 4 MXFP4 (widened to bf16)
    union {
    const uint8_t* ws4;     // MXFP4 weights: the E8M0 scale bytes in entry order [NT][KSTEPS][64][TN == 32 ? 2 : 4] (k_pack_w_fp4); else null
    const u32x4* lora_wp;   // LORA: packed bf16(scaling * B_all) [NT][lora_ksteps][64]
    };
    const float* sx;        // WQ = 3 with pre-quantised activations: xp holds int8 entries Xq[mt][kp][lane][16] (k_quant_rows_i8 / the
                            // norm kernel) and sx[b] the row absmax they were scaled by (bitsandbytes' SCA); the epilogue multiplies
                            // the int32 sum by SCA[b] / 127 * SCB[n] / 127.  k_gemm_q8: written here for the epilogue (LDS)
    int gate_rows;          // H of a gated linear_in (value row of feature n is H + n)
    union {
    float* partial;         // EPI_PARTIAL: fp32 partial sums [gridDim.y][B][N] (K split over gridDim.y workgroups so that
                            // GEMMs with few n-tiles still cover every CU); summed by k_resid_rmsnorm
    long kv_soff;           // EPI_ROPE_KV, 4-bit ring (kv8 == 2): bytes from a ring's codes plane (kc / vc) to its scale plane
    };
    // EPI_ROPE_KV (temporal in_proj): features [q | k | v], each H heads x Dh.  RoPE (rope.py:11-82, interleaved, fp32) on
    // q and k for the single new position offsets[b]; q -> qrot [B][H][Dh]; k, v -> ring slot offsets[b] % cap of
    // [B][H][cap][Dh] (RingKVCache scatter, transformer.py:243-250: written for every row, exec mask or not)
    uint16_t* qrot;
    uint16_t* kc;
    uint16_t* vc;
    const long* offsets;
    int H, Dh, cap;
    float max_period;
    const float* rope;      // [B][Dh/2][2]: (cos, sin) of the new position's angles, filled once per step by k_lm_prepare
    int kv8;                // 1: the ring holds e4m3 bytes instead of bf16 (fp8 KV cache: half the attention stream); 2: E2M1 codes
                            // [B][H][cap][Dh/2] and, kv_soff bytes behind them, E8M0 scale bytes [B][H][cap][Dh/16] (mmi_fp4.h)
    // k_gemm_xp_norm: RMSNorm of the input rows fused in front of the GEMM (xp holds the un-normalised rows)
    union {
    const uint16_t* alpha;  // [D]
    const u32x4* lora_xp;   // LORA: packed t [MT][lora_ksteps][64]
    };
    union {
    int D;                  // features of a row (the mean is over D, not the padded K)
    int lora_ksteps;        // LORA: S * R / k-step
    };
    union {
    float eps;
    int lora_slot_ksteps;   // LORA: R / k-step, the k-steps of one slot
    };
    int osplit;             // k_gemm_xp: > 1 = every n-tile is shared by `osplit` workgroups, each owning TN / 8 / osplit of its row octets
                            // (grid.x = NT * osplit).  For GEMMs with few n-tiles (N = 1024 of the depth transformer: 32 tiles on
                            // 256 CUs), where one CU cannot pull its 64-180 KB of weights faster than ~25 GB/s: a workgroup's lanes of
                            // octets it does not own repeat an owned lane's address (no extra HBM traffic; those MFMA rows are garbage
                            // that nobody writes), the epilogue writes only the owned 8-feature groups.  Not for gated epilogues.
    // per-row LoRA adapters (modules/lora.py:116-118, unmerged).  The bank of a linear holds S slots of R columns:
    // A_all [S * R][K] and bf16(scaling * B_all) [N][S * R], both packed like any weight.  A shrink launch (k_gemm_xp<.., LORA_T>,
    // MMI_EPI_LORA_T) writes t = bf16(A_all x) as a packed operand of S * R features, zero outside the row's own slot; the
    // linear itself (k_gemm_xp<.., LORA>) walks B_all against t behind its K slice, into the same accumulators.  Their
    // arguments are the lora_* / row_slot members above: each shares its bytes with a member that those launches never read
    // (bf16 linears have no ws4, k_gemm_xp no fused norm, a shrink launch no embedding), so the struct - the kernel argument of
    // every GEMM launch - is what it was
};
static_assert(sizeof(GemmArgs) == 232, "GemmArgs is the kernel argument of every GEMM launch: new arguments share bytes, they are not appended");

// The residual (or embedding) vector the thread's FIRST epilogue task will add, requested before the weight stream starts
// so that its latency is hidden behind the main loop instead of extending the epilogue.
template <int TN, int MT, int NTW>
__device__ __forceinline__ u32x4 mmi_gemm_prefetch_addend(const GemmArgs& a, int nt0) {
    u32x4 pre = {0u, 0u, 0u, 0u};
    if (a.epi != MMI_EPI_RESID && a.epi != MMI_EPI_EMB) return pre;
    const int G = TN / 8;
    const int q = (int)threadIdx.x;
    if (q >= NTW * MT * G * TN) return pre;
    const int bl = q % TN;
    int rest = q / TN;
    const int gi = rest % G;
    rest /= G;
    const int m = rest % MT, t = rest / MT;
    const int nt = nt0 + t, b = m * TN + bl, n0 = nt * TN + 8 * gi;
    if (nt >= a.NT || b >= a.B || n0 >= a.N) return pre;
    if (a.epi == MMI_EPI_RESID) {
        const uint16_t* rs = a.out_mode == MMI_OUT_PACKED ? a.resid + mmi_xp_index(TN, b, n0, a.out_ksteps) : a.resid + (long)b * a.out_ld + n0;
        pre = *reinterpret_cast<const u32x4*>(rs);
    } else {
        const int tk = a.tok[(long)(b % a.tok_rows) * a.tok_stride];
        if (tk != -1) pre = *reinterpret_cast<const u32x4*>(a.emb + (long)(tk < 0 ? 0 : tk) * a.N + n0);   // lm_utils.py:102-124
    }
    return pre;
}

// EPI_ROPE_KV, 4-bit ring: the eight bf16 ring values (k after RoPE, v as is) of the task (b, 8-feature group gi) of tile (t, m),
// re-summed from the reduction scratch exactly as that task's own thread sums them below - same wave order, same dequantisation,
// same rotation, every operation rounded on its own.  A 16-element block of the ring spans two tasks (gi, gi ^ 1): each of the
// two threads derives the partner's values itself, so both hold the same block absmax without exchanging anything - no cross-lane
// operation under the divergent `continue`s of the task loop.  The partner's sums must be real sums: the forms that hand a
// workgroup only some of a tile's row octets (GemmArgs::osplit, k_gemm_xlds) leave the other octets' accumulators meaningless,
// so the host gives a 4-bit in_proj only windows of whole octet PAIRS (plan_osplit, plan_xlds in lm_engine.hip).
template <int TN, int WAVES, int LS, int NE>
__device__ __forceinline__ void mmi_epi_kv_feats(const GemmArgs& a, const float* rb, int gi, int bl, int b, int row, int n0, bool iacc,
                                                 const float* sx_local, float* v8) {
    int off_lo, off_hi;
    if constexpr (TN == 32) { off_lo = bl * LS + 4 * gi; off_hi = (bl + 32) * LS + 4 * gi; }
    else { off_lo = (bl + 32 * gi) * LS; off_hi = (bl + 32 * gi + 16) * LS; }
    float s[8];
    if (iacc) {
        int si[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) si[e] = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const i32x4 lo = *reinterpret_cast<const i32x4*>(rb + w * NE + off_lo);
            const i32x4 hi = *reinterpret_cast<const i32x4*>(rb + w * NE + off_hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) { si[e] += lo[e]; si[4 + e] += hi[e]; }
        }
        const float sca = sx_local ? sx_local[row] : a.sx[b];
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(a.wscb + n0), c1 = *reinterpret_cast<const f32x4*>(a.wscb + n0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s[e] = mmi_i8_dequant(si[e], sca, c0[e]);
            s[4 + e] = mmi_i8_dequant(si[4 + e], sca, c1[e]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(rb + w * NE + off_lo);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(rb + w * NE + off_hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[e] += lo[e]; s[4 + e] += hi[e]; }
        }
        if (a.wscale) {
            const f32x4 c0 = *reinterpret_cast<const f32x4*>(a.wscale + n0), c1 = *reinterpret_cast<const f32x4*>(a.wscale + n0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[e] *= c0[e]; s[4 + e] *= c1[e]; }
        }
    }
    const int HD = a.H * a.Dh;
    const int sec = n0 / HD, hn = n0 - sec * HD, d0 = hn % a.Dh;
#pragma unroll
    for (int e = 0; e < 8; ++e) v8[e] = mmi_round_bf16(s[e]);
    if (sec < 2) {
        const float* cs = a.rope + ((long)b * (a.Dh / 2) + d0 / 2) * 2;
        const f32x4 cs0 = *reinterpret_cast<const f32x4*>(cs), cs1 = *reinterpret_cast<const f32x4*>(cs + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float c = j < 2 ? cs0[2 * j] : cs1[2 * j - 4], sn = j < 2 ? cs0[2 * j + 1] : cs1[2 * j - 3];
            const float re = v8[2 * j], im = v8[2 * j + 1];
            mmi_rope_rotate(re, im, c, sn, v8[2 * j], v8[2 * j + 1]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v8[e] = mmi_round_bf16(v8[e]);
}

// Split-K reduction across the workgroup's waves (fixed order -> deterministic) and the epilogue shared by the GEMM
// kernels: one task = 8 consecutive output features of one session, written as one 16-byte vector.
// EXT: the reduction scratch is handed in (`red_ext`, WAVES * NTW * MT * 64 * LS floats) instead of a static LDS array - for
// kernels that own all of the LDS themselves (k_gemm_xlds).
// g_lo / g_hi: only the tile's 8-feature groups [g_lo, g_hi) are written (k_gemm_xlds hands a tile's row octets to two
// workgroups when that balances the chip: 384 in_proj tiles over 256 CUs = 6 octets each); default = the whole tile.
// LORA_T: the shrink launch's epilogue (MMI_EPI_LORA_T) is compiled in - only into the shrink instantiations of k_gemm_xp.
// KV4: the 4-bit ring form of MMI_EPI_ROPE_KV is compiled in - only into the instantiations launch_gemm picks for the in_proj of a
// 4-bit handle (GemmArgs::kv8 == 2); every other instantiation is the code it was without that form.
template <int TN, int MT, int NTW, int WAVES, bool EXT = false, bool LORA_T = false, bool KV4 = false>
__device__ __forceinline__ void mmi_gemm_epilogue(const GemmArgs& a, float (&accv)[NTW][MT][TN == 32 ? 16 : 4], int wave, int lane,
                                                  int nt0, u32x4 pre, float* red_ext = nullptr, int g_lo = 0, int g_hi = 4,
                                                  const float* sx_local = nullptr) {
    constexpr int R = TN == 32 ? 16 : 4;
    // ---- split-K reduction across the block's waves (fixed order -> deterministic).  LDS layout [wave][tile][lane][LS]:
    // a lane's accumulators are contiguous, so they go out and come back as 16-byte vectors; LS = 20 floats (80 B)
    // spreads the 8 lanes of a ds_*_b128 group over all 32 banks.
    constexpr int LS = R == 4 ? 4 : ((WAVES * NTW * MT * 64 * 20 * 4 <= 65536) ? 20 : 16);
    constexpr int NE = NTW * MT * 64 * LS;
    float* red;
    if constexpr (EXT) {
        red = red_ext;
    } else {
        MMI_SHARED __attribute__((aligned(16))) float red_static[WAVES * NE];
        red = red_static;
    }
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int c = 0; c < R / 4; ++c) {
                const f32x4 v4 = {accv[t][m][4 * c], accv[t][m][4 * c + 1], accv[t][m][4 * c + 2], accv[t][m][4 * c + 3]};
                *reinterpret_cast<f32x4*>(&red[wave * NE + ((t * MT + m) * 64 + lane) * LS + 4 * c]) = v4;
            }
    __syncthreads();

    // ---- epilogue: one task = 8 consecutive output features of one session
    const bool gate = a.epi == MMI_EPI_GATE;
    const bool iacc = a.sx || sx_local;              // int8 x int8: accv holds int32 bit patterns
    const int rows_out = gate ? TN / 2 : TN;         // output features per tile
    const int G = rows_out / 8;                      // feature groups per tile
    const int ntasks = NTW * MT * G * TN;
    for (int q = (int)threadIdx.x; q < ntasks; q += WAVES * 64) {
        const int bl = q % TN;
        int rest = q / TN;
        const int gi = rest % G;
        rest /= G;
        const int m = rest % MT, t = rest / MT;
        const int nt = nt0 + t;
        const int b = m * TN + bl;
        const int n0 = nt * rows_out + 8 * gi;
        if (nt >= a.NT || b >= a.B || n0 >= a.N || gi < g_lo || gi >= g_hi) continue;
        const float* rb = red + (t * MT + m) * 64 * LS;
        // features 8*gi .. 8*gi+7 of the tile live in two lanes' accumulator quads (MFMA C layout, lm_kernels.h header):
        //   T = 32: rows i = 8gi+e -> register (e&3) + 4gi of lane bl + 32*(e>>2);  gate partner rows i+16 -> registers + 8
        //   T = 16: rows i = 8gi+e -> register e&3 of lane bl + 16*(2gi + (e>>2));  gate partner rows i+8 -> lanes + 32
        int off_lo, off_hi, off2_lo, off2_hi;
        if constexpr (TN == 32) {
            off_lo = bl * LS + 4 * gi; off_hi = (bl + 32) * LS + 4 * gi;
            off2_lo = off_lo + 8; off2_hi = off_hi + 8;
        } else {
            off_lo = (bl + 32 * gi) * LS; off_hi = (bl + 32 * gi + 16) * LS;
            off2_lo = (bl + 32) * LS; off2_hi = (bl + 48) * LS;
        }
        float s[8], s2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] = 0.f; s2[e] = 0.f; }
        if (iacc) {
            // int8 x int8: the waves' accumulators are int32 bit patterns; their sum is the EXACT out32 of bitsandbytes'
            // int8_linear_matmul, converted to fp32 once (round to nearest even, like `out32 * float_tensor` in torch)
            int si[8], si2[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { si[e] = 0; si2[e] = 0; }
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const i32x4 lo = *reinterpret_cast<const i32x4*>(rb + w * NE + off_lo);
                const i32x4 hi = *reinterpret_cast<const i32x4*>(rb + w * NE + off_hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) { si[e] += lo[e]; si[4 + e] += hi[e]; }
            }
            if (gate) {
#pragma unroll
                for (int w = 0; w < WAVES; ++w) {
                    const i32x4 lo = *reinterpret_cast<const i32x4*>(rb + w * NE + off2_lo);
                    const i32x4 hi = *reinterpret_cast<const i32x4*>(rb + w * NE + off2_hi);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { si2[e] += lo[e]; si2[4 + e] += hi[e]; }
                }
            }
            if (a.epi == MMI_EPI_PARTIAL) {      // split-K: the consumer (k_resid_rmsnorm) adds the integer partials, then dequantises
                int* pd = reinterpret_cast<int*>(a.partial) + ((long)blockIdx.y * a.B + b) * a.N + n0;
                *reinterpret_cast<i32x4*>(pd) = i32x4{si[0], si[1], si[2], si[3]};
                *reinterpret_cast<i32x4*>(pd + 4) = i32x4{si[4], si[5], si[6], si[7]};
                continue;
            }
            // int8_mm_dequant: out32 * (SCA[b] * SCB[n]) * (1 / 127^2), fp32, in that order
            const float sca = sx_local ? sx_local[m * TN + bl] : a.sx[b];      // sx_local: the kernel's own row absmax (LDS)
            const f32x4 c0 = *reinterpret_cast<const f32x4*>(a.wscb + n0), c1 = *reinterpret_cast<const f32x4*>(a.wscb + n0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[e] = mmi_i8_dequant(si[e], sca, c0[e]);
                s[4 + e] = mmi_i8_dequant(si[4 + e], sca, c1[e]);
            }
            if (gate) {
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.wscb + a.gate_rows + n0), g1 = *reinterpret_cast<const f32x4*>(a.wscb + a.gate_rows + n0 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s2[e] = mmi_i8_dequant(si2[e], sca, g0[e]);
                    s2[4 + e] = mmi_i8_dequant(si2[4 + e], sca, g1[e]);
                }
            }
        } else {
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(rb + w * NE + off_lo);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(rb + w * NE + off_hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[e] += lo[e]; s[4 + e] += hi[e]; }
        }
        if (gate) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(rb + w * NE + off2_lo);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(rb + w * NE + off2_hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) { s2[e] += lo[e]; s2[4 + e] += hi[e]; }
            }
        }
        }
        if (a.wscale && !iacc) {   // int8 weights, bf16 activations: y = (sum_k q x) * SCB / 127, per original weight row
            const f32x4 c0 = *reinterpret_cast<const f32x4*>(a.wscale + n0), c1 = *reinterpret_cast<const f32x4*>(a.wscale + n0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[e] *= c0[e]; s[4 + e] *= c1[e]; }
            if (gate) {
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.wscale + a.gate_rows + n0), g1 = *reinterpret_cast<const f32x4*>(a.wscale + a.gate_rows + n0 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { s2[e] *= g0[e]; s2[4 + e] *= g1[e]; }
            }
        }
        if (a.epi == MMI_EPI_PARTIAL) {
            float* pd = a.partial + ((long)blockIdx.y * a.B + b) * a.N + n0;
            f32x4 lo = {s[0], s[1], s[2], s[3]}, hi = {s[4], s[5], s[6], s[7]};
            *reinterpret_cast<f32x4*>(pd) = lo;
            *reinterpret_cast<f32x4*>(pd + 4) = hi;
            continue;
        }
        if (a.epi == MMI_EPI_DEP_QKV0) {
            // in_proj of the depth transformer's FIRST micro-step: its attention sees one position, softmax over one score is
            // exactly 1, so the attention output IS v (1 * v / 1) - the epilogue writes k and v into position 0 of the frame's
            // cache (transformer.py:243-253) and v as out_proj's packed operand; q is not needed; no attention launch
            const int HD = a.H * a.Dh;
            const int sec = n0 / HD, hn = n0 - sec * HD, h = hn / a.Dh, d0 = hn - h * a.Dh;
            if (sec == 0) continue;
            u32x4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = mmi_pack_bf16x2(s[2 * e], s[2 * e + 1]);      // nn.Linear output in bf16
            uint16_t* cache = (sec == 1 ? a.kc : a.vc) + (((long)b * a.H + h) * a.cap) * a.Dh + d0;
            *reinterpret_cast<u32x4*>(cache) = ov;
            if (sec == 2) *reinterpret_cast<u32x4*>(a.out + mmi_xp_index(TN, b, hn, a.out_ksteps)) = ov;
            continue;
        }
        if (a.epi == MMI_EPI_ROPE_KV) {
            const int HD = a.H * a.Dh;
            const int sec = n0 / HD, hn = n0 - sec * HD, h = hn / a.Dh, d0 = hn - h * a.Dh;
            const long off = a.offsets[b];
            float v8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v8[e] = mmi_round_bf16(s[e]);          // in_proj output is a bf16 tensor
            if (sec < 2) {
                const float* cs = a.rope + ((long)b * (a.Dh / 2) + d0 / 2) * 2;      // 4 (cos, sin) pairs = 32 contiguous bytes
                const f32x4 cs0 = *reinterpret_cast<const f32x4*>(cs), cs1 = *reinterpret_cast<const f32x4*>(cs + 4);
    #pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float c = j < 2 ? cs0[2 * j] : cs1[2 * j - 4], sn = j < 2 ? cs0[2 * j + 1] : cs1[2 * j - 3];
                    // mmi_rope_rotate = four multiplies, a subtract, an add as separate VALU instructions.  Written as
                    // `re * c - im * sn` the compiler packs the four pairs into v_pk_mul_f32 / v_pk_add_f32 with op_sel swizzles,
                    // one of them in place, and on gfx950 that sequence inside k_gemm_xp<32, 2, ..> (64 sessions) returned, now and
                    // then, a stale last element for lanes 48-63 - q / k of 16 sessions wrong in one feature, a different one
                    // from run to run: the "row 17" failure of the driver's round-4 suite (profiles/r05_logs/c5_trace_*.txt)
                    const float re = v8[2 * j], im = v8[2 * j + 1];
                    mmi_rope_rotate(re, im, c, sn, v8[2 * j], v8[2 * j + 1]);
                }
            }
            if constexpr (KV4) {
            if (sec != 0 && a.kv8 == 2) {
                // 4-bit ring: this task's eight values are half of a 16-element block; the other half is the task gi ^ 1 of the
                // same row (the lane bl ^ TN of this wave) - see mmi_epi_kv_feats.  Both threads quantise under the same scale
                // byte; each stores its own four code bytes, the even one the scale byte.  Vector stores.
                float mine[8], other[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) mine[e] = mmi_round_bf16(v8[e]);
                mmi_epi_kv_feats<TN, WAVES, LS, NE>(a, rb, gi ^ 1, bl, b, m * TN + bl, n0 ^ 8, iacc, sx_local, other);
                const uint32_t am0 = mmi_kv4_absmax8(mine), am1 = mmi_kv4_absmax8(other);
                const uint32_t sb = mmi_kv4_scale_byte(am0 > am1 ? am0 : am1);
                const uint32_t codes = sb ? mmi_kv4_quant8(mine, sb) : 0u;
                uint8_t* plane = reinterpret_cast<uint8_t*>(sec == 1 ? a.kc : a.vc);
                const long rowi = ((long)b * a.H + h) * a.cap + (int)(off % a.cap);
                *reinterpret_cast<uint32_t*>(plane + rowi * (a.Dh / 2) + d0 / 2) = codes;
                if (!(gi & 1)) plane[a.kv_soff + rowi * (a.Dh / 16) + d0 / 16] = (uint8_t)sb;
                continue;
            }
            }
            if (sec != 0 && a.kv8) {   // fp8 ring: the bf16 k / v values (k after RoPE, as the bf16 ring would hold them) -> e4m3
                uint8_t* d8 = reinterpret_cast<uint8_t*>(sec == 1 ? a.kc : a.vc) + (((long)b * a.H + h) * a.cap + (int)(off % a.cap)) * a.Dh + d0;
                u32x2 o8;
                o8[0] = mmi_cvt_fp8x4(mmi_round_bf16(v8[0]), mmi_round_bf16(v8[1]), mmi_round_bf16(v8[2]), mmi_round_bf16(v8[3]));
                o8[1] = mmi_cvt_fp8x4(mmi_round_bf16(v8[4]), mmi_round_bf16(v8[5]), mmi_round_bf16(v8[6]), mmi_round_bf16(v8[7]));
                *reinterpret_cast<u32x2*>(d8) = o8;
                continue;
            }
            uint16_t* dst;
            if (sec == 0) dst = a.qrot + (long)b * HD + hn;
            else dst = (sec == 1 ? a.kc : a.vc) + (((long)b * a.H + h) * a.cap + (int)(off % a.cap)) * a.Dh + d0;
            u32x4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = mmi_pack_bf16x2(v8[2 * e], v8[2 * e + 1]);
            *reinterpret_cast<u32x4*>(dst) = ov;
            continue;
        }
        if constexpr (LORA_T) {
            if (a.epi == MMI_EPI_LORA_T) {
                // t = bf16(A x), the bf16 output of lora_A (modules/lora.py:117), for the columns of the row's own slot; 0 for
                // every other slot's, so that the tail of the linear adds nothing of theirs
                const int slot = a.row_slot[b % a.tok_rows];
                u32x4 tv = {0u, 0u, 0u, 0u};
                if (slot >= 0 && n0 / a.lora_rank == slot) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) tv[e] = mmi_pack_bf16x2(s[2 * e], s[2 * e + 1]);
                }
                *reinterpret_cast<u32x4*>(a.out + mmi_xp_index(TN, b, n0, a.out_ksteps)) = tv;
                continue;
            }
        }
        uint16_t* dst = a.out_mode == MMI_OUT_PACKED ? a.out + mmi_xp_index(TN, b, n0, a.out_ksteps)
                                                     : a.out + (long)b * a.out_ld + n0;
        float o[8];
        if (gate) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float g = mmi_round_bf16(s[e]);
                const float u = mmi_round_bf16(s2[e]);
                const float act = mmi_round_bf16(g / (1.0f + expf(-g)));   // F.silu on a bf16 tensor
                o[e] = act * u;
            }
        } else if (a.epi == MMI_EPI_RESID) {
            const uint16_t* rs = a.out_mode == MMI_OUT_PACKED ? a.resid + mmi_xp_index(TN, b, n0, a.out_ksteps)
                                                              : a.resid + (long)b * a.out_ld + n0;
            const u32x4 rv = q == (int)threadIdx.x ? pre : *reinterpret_cast<const u32x4*>(rs);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint16_t h = (uint16_t)((e & 1) ? (rv[e >> 1] >> 16) : (rv[e >> 1] & 0xffffu));
                o[e] = mmi_round_bf16(s[e]) + mmi_bf16_to_f32(h);           // x_orig + update
            }
        } else if (a.epi == MMI_EPI_EMB) {
            u32x4 ev = pre;
            if (q != (int)threadIdx.x) {
                const int tk = a.tok[(long)(b % a.tok_rows) * a.tok_stride];
                ev = u32x4{0u, 0u, 0u, 0u};
                if (tk != -1) ev = *reinterpret_cast<const u32x4*>(a.emb + (long)(tk < 0 ? 0 : tk) * a.N + n0);   // lm_utils.py:102-124
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint16_t h = (uint16_t)((e & 1) ? (ev[e >> 1] >> 16) : (ev[e >> 1] & 0xffffu));
                o[e] = mmi_round_bf16(s[e]) + mmi_bf16_to_f32(h);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = s[e];                         // nn.Linear output in bf16
        }
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = mmi_pack_bf16x2(o[2 * e], o[2 * e + 1]);
        *reinterpret_cast<u32x4*>(dst) = ov;
    }
}

// MXFP4: the scale bytes of one weight entry as the lane loads them, and the byte that scales word j (k-step 4ke + j) of it
template <int TN> struct MmiFp4Scale { typedef uint16_t type; };
template <> struct MmiFp4Scale<16> { typedef uint32_t type; };
template <int TN>
__device__ __forceinline__ uint32_t mmi_fp4_scale_of(uint32_t s, int j) { return TN == 32 ? (s >> (8 * (j >> 1))) & 0xffu : (s >> (8 * j)) & 0xffu; }

// WQ = 1 (int8) / 2 (fp8) weights: one 16-byte weight entry carries two k-steps, so the loop runs over k-step PAIRS
// (a.KSTEPS then counts pairs; the activation buffers hold 2*KSTEPS k-steps, zero padded).
// WQ = 3: int8 weight entries x int8 activation entries (a.xp = Xq, one 16-byte entry per weight entry, a.sx = row absmax) on
// v_mfma_i32_{32x32x32,16x16x64}_i8; the int32 sums are converted to fp32 once per wave and go through the common epilogue.
// WQ = 4 (MXFP4): one 16-byte weight entry carries FOUR k-steps (a.KSTEPS counts entries; the activation buffers hold
// 4*KSTEPS k-steps, zero padded): the WQ = 1 loop with four activation fragments per entry.  Each word of the entry is widened
// to one bf16 fragment under its MX block's scale (mmi_fp4x8_to_bf16: 4 conversions, exact) and meets the bf16 MFMA.
// The 16-row tile (<= 16 sessions) with bf16 weights is held to 128 registers: two 8-wave workgroups per CU, so that one's
// reduction + epilogue runs under the other's weight stream (136 registers unbounded; 8 spill, outside the loop).  Same-box at
// 1 / 8 / 16 sessions: -0.12 / -0.14 / -0.12 ms per step (in_proj 20.9 -> 19.4 us, linear_in 38.4 -> 35.5, text head 48.9 ->
// 44.2; profiles/r04_logs/call_m_summary.txt).
// LORA (bf16 weights): behind its K slice the wave walks its share of the adapter bank's packed B tile against the packed t of
// the shrink launch (GemmArgs::lora_*), same MFMA, same accumulators; where K is split over gridDim.y, workgroup row 0 alone.
// The k-steps OF EACH SLOT are shared out over the waves by the main loop's rule (contiguous slices in wave order), so a wave
// adds the same share of a row's adapter whichever slot holds it - every other slot's t is +0 and changes no sum: a session's
// bits do not depend on its slot.  Everything behind the accumulators is as without it.
// LORA_T: a shrink launch (A_all against the linear's operand): the plain kernel with MMI_EPI_LORA_T compiled into its epilogue.
template <int TN, int MT, int NTW, int WAVES, int U, int WQ = 0, bool LORA = false, bool LORA_T = false, bool KV4 = false>
__global__ __launch_bounds__(WAVES * 64, (TN == 16 && MT == 1 && NTW == 1 && WQ == 0 && WAVES == 8 && !LORA && !LORA_T && !KV4) ? 4 : 1) void k_gemm_xp(GemmArgs a) {
    static_assert(!(LORA || LORA_T) || (WQ == 0 && NTW == 1), "adapters run on bf16 linears, one n-tile per workgroup");
    constexpr bool W8 = WQ == 1;
    constexpr int R = TN == 32 ? 16 : 4;          // accumulator registers per MFMA tile
    constexpr int XS = WQ == 4 ? 4 : ((WQ == 1 || WQ == 2) ? 2 : 1);   // activation fragments per weight entry
    typedef typename MmiFp4Scale<TN>::type s4_t;      // WQ = 4: the scale bytes of one entry (2 at the 32-row tile, 4 at the 16-row tile)
    typedef int iacc_t __attribute__((ext_vector_type(R)));
    typedef float acc_t __attribute__((ext_vector_type(R)));
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    // octet sharing (a.osplit > 1, NTW == 1): workgroup = (n-tile, part); part owns the 8-feature groups [g_lo, g_hi)
    const int os = (NTW == 1 && a.osplit > 1) ? a.osplit : 1;
    const int bx = (int)blockIdx.x / os, part = (int)blockIdx.x - bx * os;
    const int nt0 = bx * NTW;
    const int g_lo = part * ((TN / 8) / os), g_hi = os > 1 ? g_lo + (TN / 8) / os : TN / 8;
    // weight fragments are stored [k-step][lane], lane = (k-group, row): rows of octets the workgroup does not own are read
    // from the first owned octet instead
    const int ro = (lane >> 3) & (TN / 8 - 1);
    const int wlane = (ro >= g_lo && ro < g_hi) ? lane : ((lane & ~((TN / 8 - 1) << 3)) | (g_lo << 3));
    const u32x4 pre = mmi_gemm_prefetch_addend<TN, MT, NTW>(a, nt0);

    // K range of this workgroup (gridDim.y > 1: split-K over workgroups), then of this wave
    const int kb_per = (a.KSTEPS + (int)gridDim.y - 1) / (int)gridDim.y;
    const int kb0 = min(a.KSTEPS, (int)blockIdx.y * kb_per), kb1 = min(a.KSTEPS, kb0 + kb_per);
    const int kper = (kb1 - kb0 + WAVES - 1) / WAVES;
    const int ks0 = min(kb1, kb0 + wave * kper);
    const int nks = min(kb1, ks0 + kper) - ks0;

    const u32x4* wp[NTW];
    const u32x4* xp[MT];
#pragma unroll
    for (int t = 0; t < NTW; ++t) wp[t] = a.wp + ((long)min(nt0 + t, a.NT - 1) * a.KSTEPS + ks0) * 64 + wlane;
#pragma unroll
    for (int m = 0; m < MT; ++m) xp[m] = a.xp + ((long)m * a.KSTEPS + ks0) * XS * 64 + lane;

    acc_t acc[NTW][MT];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[t][m][r] = 0.f;

    const s4_t* sp[NTW];
    if constexpr (WQ == 4) {
#pragma unroll
        for (int t = 0; t < NTW; ++t) sp[t] = reinterpret_cast<const s4_t*>(a.ws4) + ((long)min(nt0 + t, a.NT - 1) * a.KSTEPS + ks0) * 64 + wlane;
    }
    u32x4 wA[U][NTW], xA[U][MT][XS], wB[U][NTW], xB[U][MT][XS];
    uint32_t sA[U][NTW], sB[U][NTW];                  // WQ = 4 only
#define MMI_G_LOAD(W_, X_, S_, base)                                                          \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                           \
        _Pragma("unroll") for (int t = 0; t < NTW; ++t) W_[u][t] = mmi_load_nt(wp[t] + ((base) + u) * 64); \
        if constexpr (WQ == 4) {                                                              \
            _Pragma("unroll") for (int t = 0; t < NTW; ++t) S_[u][t] = sp[t][((base) + u) * 64]; \
        }                                                                                     \
        _Pragma("unroll") for (int m = 0; m < MT; ++m)                                        \
            _Pragma("unroll") for (int x = 0; x < XS; ++x) X_[u][m][x] = xp[m][(((base) + u) * XS + x) * 64]; \
    }
#define MMI_G_MFMA(WF, XF, ACC)                                                               \
    if constexpr (TN == 32) ACC = mmi_mfma_bf16_32x32x16(WF, XF, ACC);                        \
    else ACC = mmi_mfma_bf16_16x16x32(WF, XF, ACC);
#define MMI_G_MFMA8(WF, XF, ACC)                                                              \
    if constexpr (TN == 32) ACC = mmi_mfma_fp8_32x32x16(WF, XF, ACC);                         \
    else ACC = mmi_mfma_fp8_16x16x32(WF, XF, ACC);
#define MMI_G_MMA8(W_, X_, u)                                                                 \
    {                                                                                         \
        u32x2 xq_[MT][2];                                                                     \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                      \
            xq_[m][0] = mmi_bf16x8_to_fp8(X_[u][m][0], a.xinv);                               \
            xq_[m][1] = mmi_bf16x8_to_fp8(X_[u][m][XS - 1], a.xinv);                          \
        }                                                                                     \
        _Pragma("unroll") for (int t = 0; t < NTW; ++t) {                                     \
            const u32x2 w0_ = {W_[u][t][0], W_[u][t][1]}, w1_ = {W_[u][t][2], W_[u][t][3]};   \
            _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                  \
                MMI_G_MFMA8(w0_, xq_[m][0], acc[t][m])                                        \
                MMI_G_MFMA8(w1_, xq_[m][1], acc[t][m])                                        \
            }                                                                                 \
        }                                                                                     \
    }
#define MMI_G_MMA1(W_, X_, S_, u)                                                             \
        if constexpr (WQ == 2) MMI_G_MMA8(W_, X_, u)                                          \
        else if constexpr (WQ == 4) {   /* (j & (XS - 1)) == j here: the mask only keeps this branch well-formed where XS < 4 */ \
            _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                   \
                _Pragma("unroll") for (int j = 0; j < 4; ++j) {                               \
                    const u32x4 wf_ = mmi_fp4x8_to_bf16(W_[u][t][j], mmi_fp4_scale_of<TN>(S_[u][t], j)); \
                    _Pragma("unroll") for (int m = 0; m < MT; ++m) { MMI_G_MFMA(wf_, X_[u][m][j & (XS - 1)], acc[t][m]) } \
                }                                                                             \
        } else if constexpr (WQ == 3) {                                                       \
            _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                   \
                _Pragma("unroll") for (int m = 0; m < MT; ++m) {                              \
                    if constexpr (TN == 32) acc[t][m] = __builtin_bit_cast(acc_t, mmi_mfma_i8_32x32x32(W_[u][t], X_[u][m][0], __builtin_bit_cast(iacc_t, acc[t][m]))); \
                    else acc[t][m] = __builtin_bit_cast(acc_t, mmi_mfma_i8_16x16x64(W_[u][t], X_[u][m][0], __builtin_bit_cast(iacc_t, acc[t][m]))); \
                }                                                                             \
        } else {                                                                              \
        _Pragma("unroll") for (int t = 0; t < NTW; ++t) {                                     \
            if constexpr (W8) {                                                               \
                u32x4 wlo_, whi_;                                                             \
                mmi_i8x16_to_bf16(W_[u][t], wlo_, whi_);                                      \
                _Pragma("unroll") for (int m = 0; m < MT; ++m) {                              \
                    MMI_G_MFMA(wlo_, X_[u][m][0], acc[t][m])                                  \
                    MMI_G_MFMA(whi_, X_[u][m][XS - 1], acc[t][m])                             \
                }                                                                             \
            } else {                                                                          \
                _Pragma("unroll") for (int m = 0; m < MT; ++m) { MMI_G_MFMA(W_[u][t], X_[u][m][0], acc[t][m]) } \
            }                                                                                 \
        }                                                                                     \
        }
#define MMI_G_MMA(W_, X_, S_)                                                                 \
    _Pragma("unroll") for (int u = 0; u < U; ++u) MMI_G_MMA1(W_, X_, S_, u)
    const int nfull = nks / U;
    if (nfull > 0) {
        // steady state has no conditional loads, so that the compiler's s_waitcnt vmcnt(N) before each MFMA only waits
        // for the older buffer and the loads of the next group stay in flight behind it
        MMI_G_LOAD(wA, xA, sA, 0);
        int g = 0;
        for (; g + 2 < nfull; g += 2) {
            MMI_G_LOAD(wB, xB, sB, (g + 1) * U);
            MMI_G_MMA(wA, xA, sA);
            MMI_G_LOAD(wA, xA, sA, (g + 2) * U);
            MMI_G_MMA(wB, xB, sB);
        }
        if (nfull - g == 2) {
            MMI_G_LOAD(wB, xB, sB, (g + 1) * U);
            MMI_G_MMA(wA, xA, sA);
            MMI_G_MMA(wB, xB, sB);
        } else {
            MMI_G_MMA(wA, xA, sA);
        }
    }
    // remainder of the slice (fewer than U entries): requested together - one memory round trip, not one per entry - from
    // clamped (valid) entries, and only the live ones meet the matrix core
    const int rem = nks - nfull * U;
    if (rem > 0) {
#pragma unroll
        for (int u = 0; u < U - 1; ++u) {
            const int ks = nfull * U + min(u, rem - 1);
#pragma unroll
            for (int t = 0; t < NTW; ++t) wA[u][t] = mmi_load_nt(wp[t] + ks * 64);
            if constexpr (WQ == 4) {
#pragma unroll
                for (int t = 0; t < NTW; ++t) sA[u][t] = sp[t][ks * 64];
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int x = 0; x < XS; ++x) xA[u][m][x] = xp[m][(ks * XS + x) * 64];
        }
#pragma unroll
        for (int u = 0; u < U - 1; ++u)
            if (u < rem) { MMI_G_MMA1(wA, xA, sA, u) }
    }
    if constexpr (LORA) {
        if (blockIdx.y == 0) {
            const int lks = a.lora_ksteps, rks = a.lora_slot_ksteps;
            const int lper = (rks + WAVES - 1) / WAVES;
            const int l0 = min(rks, wave * lper), lsl = min(rks, l0 + lper) - l0;     // the wave's k-steps [l0, l0 + lsl) of every slot
            const int ln = lsl * (lks / rks);
            const u32x4* lw = a.lora_wp + ((long)min(nt0, a.NT - 1) * lks + l0) * 64 + wlane;
            const u32x4* lx = a.lora_xp + l0 * 64 + lane;
            for (int g = 0; g < ln; g += U) {
                // up to U k-steps requested together, from clamped (valid) entries; only the live ones meet the matrix core
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = min(g + u, ln - 1);
                    const int ks = (i / lsl) * rks + i % lsl;
                    wA[u][0] = mmi_load_nt(lw + ks * 64);
#pragma unroll
                    for (int m = 0; m < MT; ++m) xA[u][m][0] = lx[((long)m * lks + ks) * 64];
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (g + u < ln) {
#pragma unroll
                        for (int m = 0; m < MT; ++m) { MMI_G_MFMA(wA[u][0], xA[u][m][0], acc[0][m]) }
                    }
            }
        }
    }
#undef MMI_G_LOAD
#undef MMI_G_MMA
#undef MMI_G_MMA1
#undef MMI_G_MMA8
#undef MMI_G_MFMA
#undef MMI_G_MFMA8
    float accv[NTW][MT][R];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                accv[t][m][r] = acc[t][m][r];      // WQ == 3: the wave's int32 sum, as its bit pattern (summed as integers by the epilogue)
            }
    mmi_gemm_epilogue<TN, MT, NTW, WAVES, false, LORA_T, KV4>(a, accv, wave, lane, nt0, pre, nullptr, g_lo, g_hi);
}

// k_gemm_xp for GEMMs that are a LATENCY chain, not a stream (the depth transformer's linear_out: 5.8 MB behind 128 workgroups,
// 22 k-steps per wave): the wave's WHOLE K-slice (<= KMAX k-steps: weight fragment + MT activation fragments each) is requested
// before the first MFMA - one memory round trip where the double-buffered loop of k_gemm_xp makes three (U = 4: 8 fragments in
// flight, 22 to fetch).  Same K partition over waves / workgroups, same k order inside a wave, same reduction and epilogue:
// bit-identical to k_gemm_xp<TN, MT, 1, WAVES, U>.  bf16 weights, one n-tile per workgroup, octet sharing and split-K over
// gridDim.y as in k_gemm_xp.  Registers: KMAX * (1 + MT) fragments of 4 (TN = 32, KMAX = 22: 176).
template <int TN, int MT, int WAVES, int KMAX, bool KV4 = false>
__global__ __launch_bounds__(WAVES * 64) void k_gemm_xp_once(GemmArgs a) {
    constexpr int R = TN == 32 ? 16 : 4;
    typedef float acc_t __attribute__((ext_vector_type(R)));
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int os = a.osplit > 1 ? a.osplit : 1;
    const int nt0 = (int)blockIdx.x / os, part = (int)blockIdx.x - nt0 * os;
    const int g_lo = part * ((TN / 8) / os), g_hi = os > 1 ? g_lo + (TN / 8) / os : TN / 8;
    const int ro = (lane >> 3) & (TN / 8 - 1);
    const int wlane = (ro >= g_lo && ro < g_hi) ? lane : ((lane & ~((TN / 8 - 1) << 3)) | (g_lo << 3));
    const u32x4 pre = mmi_gemm_prefetch_addend<TN, MT, 1>(a, nt0);
    const int kb_per = (a.KSTEPS + (int)gridDim.y - 1) / (int)gridDim.y;
    const int kb0 = min(a.KSTEPS, (int)blockIdx.y * kb_per), kb1 = min(a.KSTEPS, kb0 + kb_per);
    const int kper = (kb1 - kb0 + WAVES - 1) / WAVES;            // <= KMAX (checked by the launcher)
    const int ks0 = min(kb1, kb0 + wave * kper);
    const int nks = min(kb1, ks0 + kper) - ks0;
    const int ksl = min(ks0, a.KSTEPS - 1), last = nks > 0 ? nks - 1 : 0;
    const u32x4* wp = a.wp + ((long)min(nt0, a.NT - 1) * a.KSTEPS + ksl) * 64 + wlane;
    u32x4 wv[KMAX], xv[MT][KMAX];
    // unconditional loads from clamped (valid) addresses; the entries past the slice never meet the matrix core
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        const int uu = min(u, last);
        wv[u] = mmi_load_nt(wp + uu * 64);
#pragma unroll
        for (int m = 0; m < MT; ++m) xv[m][u] = a.xp[((long)m * a.KSTEPS + ksl + uu) * 64 + lane];
    }
    acc_t acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        if (u < nks) {                                           // wave-uniform
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if constexpr (TN == 32) acc[m] = mmi_mfma_bf16_32x32x16(wv[u], xv[m][u], acc[m]);
                else acc[m] = mmi_mfma_bf16_16x16x32(wv[u], xv[m][u], acc[m]);
            }
        }
    }
    float accv[1][MT][R];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) accv[0][m][r] = acc[m][r];
    mmi_gemm_epilogue<TN, MT, 1, WAVES, false, false, KV4>(a, accv, wave, lane, nt0, pre, nullptr, g_lo, g_hi);
}

// The many-row GEMM: 65..128 model rows = MT = 3 or 4 batch tiles of 32 against bf16 weights (a handle of mmi_lm_create_rows).
// Same packed operands and the same weight stream as k_gemm_xp; every weight fragment a wave loads meets all MT activation tiles
// before it is dropped, so the weights of a launch cross HBM once whatever the row count.  K is cut over gridDim.y workgroups and
// then over the workgroup's 4 waves exactly as in k_gemm_xp, each wave walks its slice in ascending k and the waves' partial
// tiles are summed in wave order: a row's sums do not depend on MT, on NTW, on the tile the row sits in or on how full the tiles
// are (MFMA columns are independent).
// NTW n-tiles per workgroup (2 for the wide GEMMs: every workgroup reads the whole MT KiB-per-k-step activation matrix from L2,
// four times the bytes of one weight tile at MT = 4, and two tiles per workgroup halve that traffic).
// Registers (MT = 4): 64 accumulators per n-tile + (NTW + MT) * 4 per fragment set in flight, two sets of U k-steps:
// NTW = 1, U = 2: 64 + 80; NTW = 2, U = 1: 128 + 48 - held under 256 so that two workgroups share a CU.
// Reduction scratch: WAVES * MT * 64 * LS floats for ONE n-tile = 64 KiB at 4 waves, MT = 4 (LS = 16) - the static array of
// mmi_gemm_epilogue.  Fewer waves (4, not 8) is what makes it fit; with NTW = 2 the tiles go through the same scratch one
// after the other (a barrier between them), not side by side.
template <int TN, int MT, int NTW, int U, bool KV4 = false>
__global__ __launch_bounds__(256, 2) void k_gemm_rows(GemmArgs a) {
    static_assert(TN == 32 && MT >= 3 && MT <= 4 && NTW >= 1 && NTW <= 2, "k_gemm_rows: 32-row tiles, 3 or 4 of them");
    constexpr int WAVES = 4, R = 16;
    typedef float acc_t __attribute__((ext_vector_type(R)));
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int nt0 = (int)blockIdx.x * NTW;
    u32x4 pre[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) pre[t] = mmi_gemm_prefetch_addend<TN, MT, 1>(a, nt0 + t);

    // K range of this workgroup (gridDim.y > 1: split-K over workgroups), then of this wave: k_gemm_xp's partition
    const int kb_per = (a.KSTEPS + (int)gridDim.y - 1) / (int)gridDim.y;
    const int kb0 = min(a.KSTEPS, (int)blockIdx.y * kb_per), kb1 = min(a.KSTEPS, kb0 + kb_per);
    const int kper = (kb1 - kb0 + WAVES - 1) / WAVES;
    const int ks0 = min(kb1, kb0 + wave * kper);
    const int nks = min(kb1, ks0 + kper) - ks0;
    const int ksl = min(ks0, a.KSTEPS - 1);          // an empty slice (nks == 0) still forms valid addresses

    const u32x4* wp[NTW];
    const u32x4* xp[MT];
#pragma unroll
    for (int t = 0; t < NTW; ++t) wp[t] = a.wp + ((long)min(nt0 + t, a.NT - 1) * a.KSTEPS + ksl) * 64 + lane;
#pragma unroll
    for (int m = 0; m < MT; ++m) xp[m] = a.xp + ((long)m * a.KSTEPS + ksl) * 64 + lane;

    acc_t acc[NTW][MT];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[t][m][r] = 0.f;

    u32x4 wA[U][NTW], xA[U][MT], wB[U][NTW], xB[U][MT];
#define MMI_R_LOAD(W_, X_, base)                                                              \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                           \
        _Pragma("unroll") for (int t = 0; t < NTW; ++t) W_[u][t] = mmi_load_nt(wp[t] + ((base) + u) * 64); \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) X_[u][m] = xp[m][((base) + u) * 64];   \
    }
#define MMI_R_MMA1(W_, X_, u)                                                                 \
    _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                           \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) acc[t][m] = mmi_mfma_bf16_32x32x16(W_[u][t], X_[u][m], acc[t][m]);
#define MMI_R_MMA(W_, X_)                                                                     \
    _Pragma("unroll") for (int u = 0; u < U; ++u) { MMI_R_MMA1(W_, X_, u) }
    const int nfull = nks / U;
    if (nfull > 0) {
        // steady state without conditional loads (see k_gemm_xp): the loads of the next group stay in flight behind the MFMAs
        MMI_R_LOAD(wA, xA, 0);
        int g = 0;
        for (; g + 2 < nfull; g += 2) {
            MMI_R_LOAD(wB, xB, (g + 1) * U);
            MMI_R_MMA(wA, xA);
            MMI_R_LOAD(wA, xA, (g + 2) * U);
            MMI_R_MMA(wB, xB);
        }
        if (nfull - g == 2) {
            MMI_R_LOAD(wB, xB, (g + 1) * U);
            MMI_R_MMA(wA, xA);
            MMI_R_MMA(wB, xB);
        } else {
            MMI_R_MMA(wA, xA);
        }
    }
    // remainder of the slice (fewer than U k-steps): loaded together from clamped (valid) entries, only the live ones multiplied
    if constexpr (U > 1) {
        const int rem = nks - nfull * U;
        if (rem > 0) {
#pragma unroll
            for (int u = 0; u < U - 1; ++u) {
                const int ks = nfull * U + min(u, rem - 1);
#pragma unroll
                for (int t = 0; t < NTW; ++t) wA[u][t] = mmi_load_nt(wp[t] + ks * 64);
#pragma unroll
                for (int m = 0; m < MT; ++m) xA[u][m] = xp[m][ks * 64];
            }
#pragma unroll
            for (int u = 0; u < U - 1; ++u)
                if (u < rem) { MMI_R_MMA1(wA, xA, u) }
        }
    }
#undef MMI_R_LOAD
#undef MMI_R_MMA
#undef MMI_R_MMA1
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        float accv[1][MT][R];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < R; ++r) accv[0][m][r] = acc[t][m][r];
        if (t > 0) __syncthreads();                  // the previous tile's sums have been read out of the scratch
        mmi_gemm_epilogue<TN, MT, 1, WAVES, false, false, KV4>(a, accv, wave, lane, nt0 + t, pre[t]);
    }
}

// RMSNorm fused into the GEMM that consumes it (the depth transformer: norm1 -> in_proj, norm2 -> linear_in; rows of
// 1024 features): y = (x.float() * (alpha.float() * rsqrt(eps + mean(x^2)))).to(bf16) (transformer.py:45-58), then
// out = y @ W^T.  A wave's whole K-slice of activation and weight fragments (<= KMAX k-steps) is loaded in one go -
// everything in flight at once, these GEMMs are latency bound - the waves combine their sums of squares through
// LDS, normalise their own fragments in registers and only then run the MFMAs.  No split-K over workgroups here.
// WQ = 1 / 2: int8 / fp8 weights, a.KSTEPS counts k-step pairs (see k_gemm_xp); KMAX = weight entries per wave.
// WQ = 4: MXFP4 weights, a.KSTEPS counts entries of four k-steps.
template <int TN, int MT, int WAVES, int KMAX, int WQ = 0>
__global__ __launch_bounds__(WAVES * 64, (TN == 16 && KMAX == 4 && WQ == 0) ? 4 : 1) void k_gemm_xp_norm(GemmArgs a) {   // 16-row tile, short rows: two workgroups per CU
    constexpr bool W8 = WQ == 1;
    constexpr int R = TN == 32 ? 16 : 4;
    constexpr int KS = TN == 32 ? 16 : 32;
    constexpr int XS = WQ == 4 ? 4 : (WQ ? 2 : 1);
    constexpr int XMAX = KMAX * XS;                           // activation fragments per wave
    typedef typename MmiFp4Scale<TN>::type s4_t;
    typedef float acc_t __attribute__((ext_vector_type(R)));
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int nt0 = (int)blockIdx.x;                          // one n-tile per workgroup (octet sharing of these GEMMs measured
    const int g_lo = 0, g_hi = TN / 8, wlane = lane;          // neutral, profiles/r02_logs/ab_osplit_norm*: not built in)
    const int kper = (a.KSTEPS + WAVES - 1) / WAVES;          // <= KMAX (checked by the launcher)
    const int ks0 = min(a.KSTEPS, wave * kper);
    const int nks = min(a.KSTEPS, ks0 + kper) - ks0;
    const int kq = TN == 32 ? (lane >> 5) : (lane >> 4);

    u32x4 wv[KMAX], xv[MT][XMAX], al[XMAX];
    uint32_t sv[KMAX];                                        // WQ = 4: the entries' scale bytes
    const u32x4 zero = {0u, 0u, 0u, 0u};
    // every load is unconditional from a clamped (valid) address and masked afterwards: conditional loads would be
    // serialised behind s_waitcnt vmcnt(0) by the compiler, and these GEMMs live on having the whole slice in flight
    const int ksl = min(ks0, a.KSTEPS - 1);
    const int dmax = (a.D - 8) > 0 ? (a.D - 8) : 0;
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        const int uu = min(u, nks > 0 ? nks - 1 : 0);
        wv[u] = mmi_load_nt(a.wp + ((long)min(nt0, a.NT - 1) * a.KSTEPS + ksl + uu) * 64 + wlane);
        if constexpr (WQ == 4) sv[u] = reinterpret_cast<const s4_t*>(a.ws4)[((long)min(nt0, a.NT - 1) * a.KSTEPS + ksl + uu) * 64 + wlane];
#pragma unroll
        for (int x = 0; x < XS; ++x) {
            const int k = ((ksl + uu) * XS + x) * KS + 8 * kq;
            al[u * XS + x] = *reinterpret_cast<const u32x4*>(a.alpha + min(k, dmax));
#pragma unroll
            for (int m = 0; m < MT; ++m) xv[m][u * XS + x] = a.xp[(((long)m * a.KSTEPS + ksl + uu) * XS + x) * 64 + lane];
        }
    }
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        const bool on = u < nks;
        if (!on) wv[u] = zero;
#pragma unroll
        for (int x = 0; x < XS; ++x) {
            const int k = ((ks0 + u) * XS + x) * KS + 8 * kq;
            if (!on || k >= a.D) al[u * XS + x] = zero;
#pragma unroll
            for (int m = 0; m < MT; ++m) if (!on) xv[m][u * XS + x] = zero;
        }
    }
    // sum of squares of this lane's row over the wave's slice (the kq lane groups hold different k of the same row)
    MMI_SHARED float ssum[WAVES][MT][TN];
    float rs[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        float ss = 0.f;
#pragma unroll
        for (int u = 0; u < XMAX; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float lo = mmi_bf16_to_f32((uint16_t)(xv[m][u][q] & 0xffffu)), hi = mmi_bf16_to_f32((uint16_t)(xv[m][u][q] >> 16));
                ss += lo * lo;
                ss += hi * hi;
            }
        if constexpr (TN == 32) ss += mmi_shfl_xor(ss, 32);
        else { ss += mmi_shfl_xor(ss, 16); ss += mmi_shfl_xor(ss, 32); }
        if (lane < TN) ssum[wave][m][lane] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) tot += ssum[w][m][lane & (TN - 1)];
        rs[m] = mmi_rsqrtf(a.eps + tot / (float)a.D);
    }
    acc_t acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        u32x4 wf[XS];
        if constexpr (W8) mmi_i8x16_to_bf16(wv[u], wf[0], wf[XS - 1]);
        else if constexpr (WQ == 4) {       // (a masked entry is zero codes: zero under any scale)
#pragma unroll
            for (int x = 0; x < XS; ++x) wf[x] = mmi_fp4x8_to_bf16(wv[u][x], mmi_fp4_scale_of<TN>(sv[u], x));
        } else wf[0] = wv[u];
        const u32x2 w8f[2] = {{wv[u][0], wv[u][1]}, {wv[u][2], wv[u][3]}};   // fp8: the two k-steps of the entry
#pragma unroll
        for (int x = 0; x < XS; ++x) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                u32x4 xn;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const u32x4& xr = xv[m][u * XS + x];
                    const u32x4& ar = al[u * XS + x];
                    const float lo = mmi_bf16_to_f32((uint16_t)(xr[q] & 0xffffu)), hi = mmi_bf16_to_f32((uint16_t)(xr[q] >> 16));
                    const float alo = mmi_bf16_to_f32((uint16_t)(ar[q] & 0xffffu)), ahi = mmi_bf16_to_f32((uint16_t)(ar[q] >> 16));
                    xn[q] = mmi_pack_bf16x2(lo * (alo * rs[m]), hi * (ahi * rs[m]));
                }
                if constexpr (WQ == 2) {        // the norm output is a bf16 tensor; it is that tensor the linear quantises
                    const u32x2 x8 = mmi_bf16x8_to_fp8(xn, a.xinv);
                    if constexpr (TN == 32) acc[m] = mmi_mfma_fp8_32x32x16(w8f[x], x8, acc[m]);
                    else acc[m] = mmi_mfma_fp8_16x16x32(w8f[x], x8, acc[m]);
                } else if constexpr (TN == 32) acc[m] = mmi_mfma_bf16_32x32x16(wf[x], xn, acc[m]);
                else acc[m] = mmi_mfma_bf16_16x16x32(wf[x], xn, acc[m]);
            }
        }
    }
    float accv[1][MT][R];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            accv[0][m][r] = acc[m][r];
        }
    mmi_gemm_epilogue<TN, MT, 1, WAVES>(a, accv, wave, lane, nt0, u32x4{0u, 0u, 0u, 0u}, nullptr, g_lo, g_hi);
}

// int8 weights x int8 activations with the row quantisation INSIDE the GEMM (the depth transformer's linears, whose rows are
// short enough - <= 8 * KMAX entries of 32 / 64 k - for one workgroup to hold): bitsandbytes' int8_vectorwise_quant needs the
// absmax of the WHOLE input row, and every workgroup of these N-split GEMMs reads the whole row anyway, so each derives it
// itself - no extra launch on the depth transformer's dependent chain, no cross-workgroup traffic.  Per batch tile: the wave's
// bf16 fragments are loaded in one go, (NORM: RMSNorm'ed in registers exactly as k_gemm_xp_norm does - the norm's output is the
// bf16 tensor the linear quantises,) the block reduces the rows' absmax through LDS, every lane converts its own fragments
// (round half even) and feeds v_mfma_i32_{32x32x32,16x16x64}_i8; the epilogue scales the int32 sums by SCA[b] * SCB[n] / 127^2.
// a.KSTEPS counts weight entries (two bf16 k-steps each).
// gridDim.y > 1 (MT == 1 only): ONE BATCH TILE PER WORKGROUP - blockIdx.y picks the tile, and the workgroup sees the GEMM of those
// TN rows alone (operand, output, residual, frame-cache pointers moved to the tile; B = the rows it holds).  At 33..64 sessions the
// MT = 2 form walks the two tiles one after the other through the same registers, three barriers each, on a latency-bound chain
// (dep.ffn_out 19.5 us against 8.2 for the bf16 kernel at 32 sessions, profiles/r04_q8_b64_sites.csv); the weights are 3-6 MB per
// linear and a tile's second reader finds them in its XCD's L2 (grid.x is a multiple of 8: both readers of an n-tile share an XCD).
template <int TN>
__device__ __forceinline__ void mmi_gemm_batch_tile_view(GemmArgs& a, int y, int x_frags_per_tile) {
    const int r0 = y * TN;
    a.xp += (long)y * x_frags_per_tile * 64;
    const long oshift = a.out_mode == MMI_OUT_PACKED ? (long)y * a.out_ksteps * 512 : (long)r0 * a.out_ld;
    if (a.out) a.out += oshift;
    if (a.resid) a.resid += oshift;
    if (a.kc) { a.kc += (long)r0 * a.H * a.cap * a.Dh; a.vc += (long)r0 * a.H * a.cap * a.Dh; }
    a.B = min(TN, a.B - r0);
}

template <int TN, int MT, int WAVES, int KMAX, bool NORM>
__global__ __launch_bounds__(WAVES * 64) void k_gemm_q8(GemmArgs a_in) {
    GemmArgs a = a_in;
    if constexpr (MT == 1) { if (gridDim.y > 1) mmi_gemm_batch_tile_view<TN>(a, (int)blockIdx.y, a.KSTEPS * 2); }
    constexpr int R = TN == 32 ? 16 : 4;
    constexpr int KS = TN == 32 ? 16 : 32;
    constexpr int XMAX = 2 * KMAX;
    // batch tiles handled together: both while a lane's fragments of both fit its registers (short rows), else one after the other
    constexpr int MG = (MT * XMAX <= 16) ? MT : 1;
    typedef int iacc_t __attribute__((ext_vector_type(R)));
    typedef float facc_t __attribute__((ext_vector_type(R)));
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    // octet sharing as in k_gemm_xp (a.osplit > 1): N = 1024 linears have 32 n-tiles for 256 CUs; a workgroup = (tile, part) owns
    // TN / 8 / osplit of the tile's 8-row groups, the lanes of the other groups repeat an owned lane's weight address
    const int os = a.osplit > 1 ? a.osplit : 1;
    const int nt0 = (int)blockIdx.x / os, part = (int)blockIdx.x - nt0 * os;
    const int g_lo = part * ((TN / 8) / os), g_hi = os > 1 ? g_lo + (TN / 8) / os : TN / 8;
    const int ro = (lane >> 3) & (TN / 8 - 1);
    const int wlane = (ro >= g_lo && ro < g_hi) ? lane : ((lane & ~((TN / 8 - 1) << 3)) | (g_lo << 3));
    const int kper = (a.KSTEPS + WAVES - 1) / WAVES;          // <= KMAX (checked by the launcher)
    const int ks0 = min(a.KSTEPS, wave * kper);
    const int nks = min(a.KSTEPS, ks0 + kper) - ks0;
    const int kq = TN == 32 ? (lane >> 5) : (lane >> 4);
    const u32x4 pre = mmi_gemm_prefetch_addend<TN, MT, 1>(a, nt0);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const int ksl = min(ks0, a.KSTEPS - 1);
    u32x4 wv[KMAX];
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        const int uu = min(u, nks > 0 ? nks - 1 : 0);
        wv[u] = mmi_load_nt(a.wp + ((long)min(nt0, a.NT - 1) * a.KSTEPS + ksl + uu) * 64 + wlane);
    }
#pragma unroll
    for (int u = 0; u < KMAX; ++u) if (u >= nks) wv[u] = zero;
    MMI_SHARED float sxl[MT * TN];                       // the rows' absmax, for the epilogue
    MMI_SHARED float redl[2][WAVES][MG][TN];             // [0] sums of squares, [1] absmax, per wave and tile of the group
    iacc_t acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0;
    const int dmax = (a.D - 8) > 0 ? (a.D - 8) : 0;
    u32x4 al[NORM ? XMAX : 1];
    if constexpr (NORM) {
#pragma unroll
        for (int u = 0; u < XMAX; ++u) {
            const int uu = min(u >> 1, nks > 0 ? nks - 1 : 0);
            al[u] = *reinterpret_cast<const u32x4*>(a.alpha + min(((ksl + uu) * 2 + (u & 1)) * KS + 8 * kq, dmax));
        }
#pragma unroll
        for (int u = 0; u < XMAX; ++u)
            if ((u >> 1) >= nks || ((ks0 + (u >> 1)) * 2 + (u & 1)) * KS + 8 * kq >= a.D) al[u] = zero;
    }
#pragma unroll
    for (int m0 = 0; m0 < MT; m0 += MG) {
        // unconditional loads from clamped (valid) addresses, masked afterwards (a load under a branch would be serialised)
        u32x4 xv[MG][XMAX];
#pragma unroll
        for (int g = 0; g < MG; ++g)
#pragma unroll
            for (int u = 0; u < XMAX; ++u) {
                const int uu = min(u >> 1, nks > 0 ? nks - 1 : 0);
                xv[g][u] = a.xp[(((long)(m0 + g) * a.KSTEPS + ksl + uu) * 2 + (u & 1)) * 64 + lane];
            }
#pragma unroll
        for (int g = 0; g < MG; ++g)
#pragma unroll
            for (int u = 0; u < XMAX; ++u)
                if ((u >> 1) >= nks) xv[g][u] = zero;
        if constexpr (NORM) {       // y = (x.float() * (alpha.float() * rsqrt(eps + mean(x^2)))).to(bf16)   (transformer.py:45-58)
#pragma unroll
            for (int g = 0; g < MG; ++g) {
                float ss = 0.f;
#pragma unroll
                for (int u = 0; u < XMAX; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float lo = mmi_bf16_to_f32((uint16_t)(xv[g][u][q] & 0xffffu)), hi = mmi_bf16_to_f32((uint16_t)(xv[g][u][q] >> 16));
                        ss += lo * lo;
                        ss += hi * hi;
                    }
                if constexpr (TN == 32) ss += mmi_shfl_xor(ss, 32);
                else { ss += mmi_shfl_xor(ss, 16); ss += mmi_shfl_xor(ss, 32); }
                if (lane < TN) redl[0][wave][g][lane] = ss;
            }
            __syncthreads();
#pragma unroll
            for (int g = 0; g < MG; ++g) {
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) tot += redl[0][w][g][lane & (TN - 1)];
                const float rs = mmi_rsqrtf(a.eps + tot / (float)a.D);
#pragma unroll
                for (int u = 0; u < XMAX; ++u) {
                    u32x4 xn;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float lo = mmi_bf16_to_f32((uint16_t)(xv[g][u][q] & 0xffffu)), hi = mmi_bf16_to_f32((uint16_t)(xv[g][u][q] >> 16));
                        const float alo = mmi_bf16_to_f32((uint16_t)(al[u][q] & 0xffffu)), ahi = mmi_bf16_to_f32((uint16_t)(al[u][q] >> 16));
                        xn[q] = mmi_pack_bf16x2(lo * (alo * rs), hi * (ahi * rs));
                    }
                    xv[g][u] = xn;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < MG; ++g) {
            float am = 0.f;
#pragma unroll
            for (int u = 0; u < XMAX; ++u) am = fmaxf(am, mmi_absmax_bf16x8(xv[g][u]));
            if constexpr (TN == 32) am = fmaxf(am, mmi_shfl_xor(am, 32));
            else { am = fmaxf(am, mmi_shfl_xor(am, 16)); am = fmaxf(am, mmi_shfl_xor(am, 32)); }
            if (lane < TN) redl[1][wave][g][lane] = am;
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < MG; ++g) {
            float sca = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) sca = fmaxf(sca, redl[1][w][g][lane & (TN - 1)]);
            if (wave == 0 && lane < TN) sxl[(m0 + g) * TN + lane] = sca;
            const float scale = mmi_i8_scale(sca);
#pragma unroll
            for (int u = 0; u < KMAX; ++u) {
                const u32x2 qlo = mmi_quant_i8x8(xv[g][2 * u], scale), qhi = mmi_quant_i8x8(xv[g][2 * u + 1], scale);
                const u32x4 xq = {qlo[0], qlo[1], qhi[0], qhi[1]};
                if constexpr (TN == 32) acc[m0 + g] = mmi_mfma_i8_32x32x32(wv[u], xq, acc[m0 + g]);
                else acc[m0 + g] = mmi_mfma_i8_16x16x64(wv[u], xq, acc[m0 + g]);
            }
        }
        __syncthreads();                                 // redl is rewritten by the next group; sxl is read by the epilogue
    }
    float accv[1][MT][R];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) accv[0][m][r] = __builtin_bit_cast(facc_t, acc[m])[r];     // int32 bit patterns (see the epilogue)
    mmi_gemm_epilogue<TN, MT, 1, WAVES>(a, accv, wave, lane, nt0, pre, nullptr, g_lo, g_hi, sxl);
}

// ------------------------------------------------------------------------------------------------
// weight-streaming GEMM with the activations resident in LDS
// ------------------------------------------------------------------------------------------------
// k_gemm_xp re-reads the whole activation matrix from L2 in every workgroup (one per n-tile): at 32 sessions that is as many
// L2 bytes as the weights themselves, at 64 twice as many, and the L2 (about 10-11 TB/s of 128-byte requests) - not HBM -
// becomes the bound (profiles/r01_pmc_sq_tcc_ffn_in_b32_b64.csv).  Here ONE workgroup per CU walks a contiguous
// range of up to NTMAX n-tiles.  K is cut into chunks of KC k-steps whose activation fragments (MT x KC KiB) are staged in LDS,
// double-buffered, so every activation byte leaves the L2 once per workgroup; the 8 waves split a chunk's k-steps, stream their
// KPW weight fragments per (chunk, tile) segment from HBM one segment ahead of the MFMAs (register double buffer) and read
// the activation fragments with ds_read_b128.  The tiles' accumulators stay in registers across the chunks; at the end each
// tile goes through the common split-K reduction + epilogue, with the reduction scratch laid over the (then idle) chunk buffers.
// Prototype in scripts/gemm_microbench.hip (main loop only): 31.7 us against 34.8 us at 32 sessions, 37.4 against 51 us at 64.
// bf16 weights, 32-row tiles.  Dynamic LDS = max(2 * MT * KC KiB, reduction scratch); a.KSTEPS % KC == 0.
// STAGGER (MMI_GEMM_LDS=2, not yet measured on hardware): in the LAST chunk each tile's reduction + epilogue runs right after
// its MFMAs, on the chunk buffer that is idle by then, while the next tile's weights (requested before those MFMAs) are still
// streaming - instead of all the tiles' epilogues one after the other behind a finished weight stream.
struct MmiTrue { static constexpr bool value = true; };
struct MmiFalse { static constexpr bool value = false; };
// WQ = 1 / 2: int8 / fp8 weight entries (two k-steps per 16-byte entry, see k_gemm_xp): KC and a.KSTEPS count ENTRIES and every
// entry meets XS = 2 activation fragments, so the production chunk is 32 / MT entries (the same 64 KiB of activations).
// Chunks shorter than 8 entries (the tiny shapes of the tests) leave the upper waves without k-steps: they keep zero
// accumulators and only take part in the barriers and the epilogue.
template <int MT, int KC, int NTMAX = 3, bool STAGGER = false, int WQ = 0, bool KV4 = false>
__global__ __launch_bounds__(512) void k_gemm_xlds(GemmArgs a) {
    typedef float acc_t __attribute__((ext_vector_type(16)));
    constexpr int XS = (WQ == 1 || WQ == 2) ? 2 : 1;   // activation fragments per weight entry (WQ = 3: int8 entries, one each)
    constexpr int KPW = KC >= 8 ? KC / 8 : 1;   // entries per wave per chunk
    constexpr int ACTIVE = KC / KPW;            // waves that own k-steps
    constexpr int XE = MT * KC * XS * 64;       // 16-byte activation pieces per chunk
    constexpr int XPT = (XE + 511) / 512;       // ... per thread
    static_assert(KC % KPW == 0 && ACTIVE <= 8, "a chunk is split over at most 8 waves");
    MMI_DYN_SHARED(u32x4, xs);                  // [2][XE], later the reduction scratch
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool active = ACTIVE == 8 || wave < ACTIVE;
    const int wk = active ? wave : 0;           // idle waves point at valid addresses and never load
    const int G = (int)gridDim.x, bid = (int)blockIdx.x;
    // The workgroup's share of the n-tiles, in row OCTETS (8 of a tile's 32 weight rows) when the epilogue writes 8-feature
    // groups that map one to one onto them (everything but the gated linear_in, whose tiles interleave gate and value rows):
    // 384 in_proj tiles over 256 workgroups are 6 octets = 1.5 tiles each instead of 1 or 2 whole tiles, i.e. every CU streams
    // the same number of bytes.  A workgroup that owns only part of a tile loads only those octets' lanes (the other lanes
    // repeat a valid lane's address: rows of the MFMA are independent, their results are simply not written).
    const bool by_octet = a.epi != MMI_EPI_GATE;
    const long units = by_octet ? 4L * a.NT : (long)a.NT;
    const long u0 = (long)bid * units / G, u1 = (long)(bid + 1) * units / G;          // [u0, u1) octets or tiles
    const int t0 = by_octet ? (int)(u0 >> 2) : (int)u0;
    const int t1 = by_octet ? (int)((u1 + 3) >> 2) : (int)u1;
    const int ntiles = u1 > u0 ? t1 - t0 : 0;   // <= NTMAX (the launcher sizes the grid)
    // octet window of tile t0 + t
    auto oct_lo = [&](int t) { return by_octet ? (int)max(0L, u0 - 4L * (t0 + t)) : 0; };
    auto oct_hi = [&](int t) { return by_octet ? (int)min(4L, u1 - 4L * (t0 + t)) : 4; };
    const int nchunks = a.KSTEPS / KC;
    acc_t acc[NTMAX][MT];
#pragma unroll
    for (int t = 0; t < NTMAX; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][m][r] = 0.f;
    // chunk c of the packed activations Xp[m][ks][lane] (XS fragments per entry) -> xs[buf][((m * KC + k) * XS + x) * 64 + lane]
    auto xsrc = [&](int c, int e) {
        const int m = e / (KC * XS * 64), rest = e - m * (KC * XS * 64);
        return a.xp + ((long)m * a.KSTEPS + (long)c * KC) * XS * 64 + rest;
    };
    u32x4 xpre[XPT];
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
        const int e = min(j * 512 + tid, XE - 1);
        xpre[j] = *xsrc(0, e);
    }
#pragma unroll
    for (int j = 0; j < XPT; ++j)
        if (j * 512 + tid < XE) xs[j * 512 + tid] = xpre[j];
    auto wsrc = [&](int c, int t) {
        const int ro = (lane >> 3) & 3, lo = oct_lo(t), hi = oct_hi(t);
        const int ln = (ro >= lo && ro < hi) ? lane : ((lane & ~0x18) | (lo << 3));       // lanes of octets it does not own
        return a.wp + ((long)min(t0 + t, a.NT - 1) * a.KSTEPS + (long)c * KC + wk * KPW) * 64 + ln;
    };
    u32x4 cur[KPW], nxt[KPW];
    if (active) {
        const u32x4* wp = wsrc(0, 0);
#pragma unroll
        for (int i = 0; i < KPW; ++i) cur[i] = mmi_load_nt(wp + i * 64);
    }
    // one weight entry against the resident activations
    auto mma = [&](const u32x4& w, const u32x4* xe, acc_t (&ac)[MT]) {
        if constexpr (WQ == 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m) ac[m] = mmi_mfma_bf16_32x32x16(w, xe[m * KC * XS * 64], ac[m]);
        } else if constexpr (WQ == 3) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
                ac[m] = __builtin_bit_cast(acc_t, mmi_mfma_i8_32x32x32(w, xe[m * KC * XS * 64], __builtin_bit_cast(i32x16, ac[m])));
        } else if constexpr (WQ == 1) {
            u32x4 lo, hi;
            mmi_i8x16_to_bf16(w, lo, hi);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                ac[m] = mmi_mfma_bf16_32x32x16(lo, xe[m * KC * XS * 64], ac[m]);
                ac[m] = mmi_mfma_bf16_32x32x16(hi, xe[m * KC * XS * 64 + 64], ac[m]);
            }
        } else {
            const u32x2 w0 = {w[0], w[1]}, w1 = {w[2], w[3]};
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                ac[m] = mmi_mfma_fp8_32x32x16(w0, mmi_bf16x8_to_fp8(xe[m * KC * XS * 64], a.xinv), ac[m]);
                ac[m] = mmi_mfma_fp8_32x32x16(w1, mmi_bf16x8_to_fp8(xe[m * KC * XS * 64 + 64], a.xinv), ac[m]);
            }
        }
    };
    // one chunk: LAST = the final chunk (nothing to prefetch; with STAGGER each tile's epilogue follows its MFMAs at once)
    auto run_chunk = [&](int c, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        __syncthreads();                        // chunk c is in xs[c & 1]; nobody reads xs[(c + 1) & 1] any more
        if constexpr (!LAST) {
#pragma unroll
            for (int j = 0; j < XPT; ++j) {
                const int e = min(j * 512 + tid, XE - 1);
                xpre[j] = *xsrc(c + 1, e);
            }
        }
        const u32x4* xb = xs + (c & 1) * XE + wk * KPW * XS * 64 + lane;
#pragma unroll
        for (int t = 0; t < NTMAX; ++t) {
            if (t < ntiles) {
                if (active) {
                    // the weights of the NEXT segment - (chunk c, tile t + 1), or (chunk c + 1, first tile) - are requested first
                    const bool last_tile = t == ntiles - 1;
                    const int nc = min(last_tile ? c + 1 : c, nchunks - 1), nt = last_tile ? 0 : t + 1;
                    const u32x4* wp = wsrc(nc, nt);
#pragma unroll
                    for (int i = 0; i < KPW; ++i) nxt[i] = mmi_load_nt(wp + i * 64);
#pragma unroll
                    for (int i = 0; i < KPW; ++i) mma(cur[i], xb + i * XS * 64, acc[t]);
#pragma unroll
                    for (int i = 0; i < KPW; ++i) cur[i] = nxt[i];
                }
                if constexpr (STAGGER && LAST) {
                    // scratch: the other chunk buffer (last read before this chunk's opening barrier, not refilled any more);
                    // the small test chunks are smaller than the scratch, which then sits behind both buffers
                    float* red = reinterpret_cast<float*>(XE * 16 >= 65536 ? xs + (nchunks & 1) * XE : xs + 2 * XE);
                    __syncthreads();            // the previous tile's output tasks are done with the scratch
                    float accv[1][MT][16];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int r = 0; r < 16; ++r) accv[0][m][r] = acc[t][m][r];
                    mmi_gemm_epilogue<32, MT, 1, 8, true, false, KV4>(a, accv, wave, lane, t0 + t, u32x4{0u, 0u, 0u, 0u}, red, oct_lo(t), oct_hi(t));
                }
            }
        }
        if constexpr (!LAST) {
#pragma unroll
            for (int j = 0; j < XPT; ++j)
                if (j * 512 + tid < XE) xs[((c + 1) & 1) * XE + j * 512 + tid] = xpre[j];
        }
    };
    for (int c = 0; c + 1 < nchunks; ++c) run_chunk(c, MmiFalse{});
    run_chunk(nchunks - 1, MmiTrue{});
    if constexpr (STAGGER) return;
    // ---- per tile: split-K reduction over the 8 waves + the common epilogue; the scratch overlays the chunk buffers
    float* red = reinterpret_cast<float*>(xs);
#pragma unroll
    for (int t = 0; t < NTMAX; ++t) {
        if (t < ntiles) {
            __syncthreads();                    // the chunk buffers / the previous tile's scratch are no longer read
            float accv[1][MT][16];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) accv[0][m][r] = acc[t][m][r];     // WQ == 3: int32 bit patterns (see the epilogue)
            mmi_gemm_epilogue<32, MT, 1, 8, true, false, KV4>(a, accv, wave, lane, t0 + t, u32x4{0u, 0u, 0u, 0u}, red, oct_lo(t), oct_hi(t));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// RMSNorm (rms_norm_f32, eps 1e-8): y = (x.float() * (alpha.float() * rsqrt(eps + mean(x^2)))).to(bf16)
// ------------------------------------------------------------------------------------------------
// One block per session row b; thread t owns the 16-byte piece (8 features) t, t + blockDim, ... of the packed row
// (launch with blockDim = D/8 up to 1024 so that a row is a single round of loads held in registers).
// P > 0: first finish the preceding split-K GEMM (out_proj / linear_out) and its residual connection,
//        x <- x + bf16(sum_p partial[p][b][:])      (transformer.py:739-741,772-776: x_orig + update, bf16 tensors)
// then   y <- rms_norm_f32(x) * alpha               (transformer.py:45-58)
#define MMI_NORM_MAXP 4      // pieces per thread kept in registers (D <= 8 * 1024 * MMI_NORM_MAXP)
// yq != null (int8 activations): the normalised row is also stored quantised row-wise for the int8 linears that read it -
// Xq[mt][kp][lane][16] (the bytes of k-steps 2 kp and 2 kp + 1) and sx[b] = its absmax (bitsandbytes' CA / SCA).
__global__ __launch_bounds__(1024) void k_resid_rmsnorm(uint16_t* __restrict__ x, const float* __restrict__ partial, int P,
                                                        int B, const uint16_t* __restrict__ alpha, uint16_t* __restrict__ y,
                                                        int D, int T, int ksteps, float eps, uint8_t* __restrict__ yq = nullptr,
                                                        float* __restrict__ sx = nullptr, const float* __restrict__ psx = nullptr,
                                                        const float* __restrict__ pscb = nullptr) {
    // psx / pscb != null: the pending GEMM was int8 x int8 - its partials are int32 sums (the exact out32 once added), and the
    // dequantisation out32 * (SCA[b] * SCB[n]) / 127^2 happens here (psx = the absmax of that GEMM's input rows, pscb = its SCB)
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    float f[MMI_NORM_MAXP][8];
    u32x4 al[MMI_NORM_MAXP];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
        const long at = mmi_xp_index(T, b, i, ksteps);
        u32x4 v = *reinterpret_cast<const u32x4*>(x + at);
        al[j] = *reinterpret_cast<const u32x4*>(alpha + i);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f[j][2 * q] = mmi_bf16_to_f32((uint16_t)(v[q] & 0xffffu));
            f[j][2 * q + 1] = mmi_bf16_to_f32((uint16_t)(v[q] >> 16));
        }
        if (P > 0) {
            float u[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) u[e] = 0.f;
            f32x4 plo[4], phi[4];                                  // P <= 4; unconditional (clamped) loads, all in flight
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float* pp = partial + ((long)min(p, P - 1) * B + b) * D + i;
                plo[p] = *reinterpret_cast<const f32x4*>(pp);
                phi[p] = *reinterpret_cast<const f32x4*>(pp + 4);
            }
            if (psx) {
                int si[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) si[e] = 0;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (p < P) {
                        const i32x4 ilo = __builtin_bit_cast(i32x4, plo[p]), ihi = __builtin_bit_cast(i32x4, phi[p]);   // (whole vectors:
#pragma unroll                                                                                                      // an element-wise
                        for (int e = 0; e < 4; ++e) { si[e] += ilo[e]; si[4 + e] += ihi[e]; }                            // bit_cast is not)
                    }
                }
                const float sca = psx[b];
                const f32x4 c0 = *reinterpret_cast<const f32x4*>(pscb + i), c1 = *reinterpret_cast<const f32x4*>(pscb + i + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { u[e] = mmi_i8_dequant(si[e], sca, c0[e]); u[4 + e] = mmi_i8_dequant(si[4 + e], sca, c1[e]); }
            } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float on = p < P ? 1.f : 0.f;                // exact: x*1 = x, finite x*0 = 0
#pragma unroll
                for (int e = 0; e < 4; ++e) { u[e] += plo[p][e] * on; u[4 + e] += phi[p][e] * on; }
            }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) f[j][e] = mmi_round_bf16(mmi_round_bf16(u[e]) + f[j][e]);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = mmi_pack_bf16x2(f[j][2 * q], f[j][2 * q + 1]);
            *reinterpret_cast<u32x4*>(x + at) = v;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += f[j][e] * f[j][e];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += mmi_shfl_xor(ss, m);
    MMI_SHARED float red[16];
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < (nth + 63) / 64; ++w) tot += red[w];
    const float rs = mmi_rsqrtf(eps + tot / (float)D);
    u32x4 ov[MMI_NORM_MAXP];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float alo = mmi_bf16_to_f32((uint16_t)(al[j][q] & 0xffffu)), ahi = mmi_bf16_to_f32((uint16_t)(al[j][q] >> 16));
            o[q] = mmi_pack_bf16x2(f[j][2 * q] * (alo * rs), f[j][2 * q + 1] * (ahi * rs));
        }
        *reinterpret_cast<u32x4*>(y + mmi_xp_index(T, b, i, ksteps)) = o;
        ov[j] = o;
        am = fmaxf(am, mmi_absmax_bf16x8(o));
    }
    if (!yq) return;
    // ---- row-wise int8 copy of the normalised row
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) am = fmaxf(am, mmi_shfl_xor(am, m));
    MMI_SHARED float redm[16];
    if ((tid & 63) == 0) redm[tid >> 6] = am;
    __syncthreads();
    float sca = 0.f;
    for (int w = 0; w < (nth + 63) / 64; ++w) sca = fmaxf(sca, redm[w]);
    if (tid == 0) sx[b] = sca;
    const float scale = mmi_i8_scale(sca);
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
        const long at = mmi_xp_index(T, b, i, ksteps);            // bf16 element index of the piece: fragment (mt * ksteps + ks), lane
        const long frag = at >> 9;
        const int ln = (int)((at >> 3) & 63);
        const long mt = frag / ksteps;
        const int ks = (int)(frag - mt * ksteps);
        *reinterpret_cast<u32x2*>(yq + ((mt * (ksteps >> 1) + (ks >> 1)) * 64 + ln) * 16 + (ks & 1) * 8) = mmi_quant_i8x8(ov[j], scale);
    }
}

// A packed bf16 tensor [B][D] -> its row-wise int8 copy Xq[mt][kp][lane][16] + the rows' absmax sx[b] (bitsandbytes'
// int8_vectorwise_quant), for the int8 linears whose input is written by MANY workgroups (the temporal attention output, the
// gated FFN tensor): one workgroup per row holds the row in registers (as the norm kernel does), reduces the absmax, converts.
__global__ __launch_bounds__(1024) void k_quant_rows_i8(const uint16_t* __restrict__ x, int B, int D, int T, int ksteps,
                                                        uint8_t* __restrict__ xq, float* __restrict__ sx) {
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    u32x4 v[MMI_NORM_MAXP];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
        v[j] = *reinterpret_cast<const u32x4*>(x + mmi_xp_index(T, b, i, ksteps));
        am = fmaxf(am, mmi_absmax_bf16x8(v[j]));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) am = fmaxf(am, mmi_shfl_xor(am, m));
    MMI_SHARED float redm[16];
    if ((tid & 63) == 0) redm[tid >> 6] = am;
    __syncthreads();
    float sca = 0.f;
    for (int w = 0; w < (nth + 63) / 64; ++w) sca = fmaxf(sca, redm[w]);
    if (tid == 0) sx[b] = sca;
    const float scale = mmi_i8_scale(sca);
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
        const long at = mmi_xp_index(T, b, i, ksteps);
        const long frag = at >> 9;
        const int ln = (int)((at >> 3) & 63);
        const long mt = frag / ksteps;
        const int ks = (int)(frag - mt * ksteps);
        *reinterpret_cast<u32x2*>(xq + ((mt * (ksteps >> 1) + (ks >> 1)) * 64 + ln) * 16 + (ks & 1) * 8) = mmi_quant_i8x8(v[j], scale);
    }
}

// The cross-attention block's norm (transformer.py:731-732, 779-783: `norm_cross` is always an nn.LayerNorm with weight and
// bias, eps 1e-5): same row handling as k_resid_rmsnorm - first fold the P pending split-K partials of the preceding out_proj
// into the residual stream - then y = ((x - mean) * rsqrt(var + eps) * w + b).to(bf16), statistics in fp32 over the D features.
__global__ __launch_bounds__(1024) void k_resid_layernorm(uint16_t* __restrict__ x, const float* __restrict__ partial, int P,
                                                          int B, const uint16_t* __restrict__ w, const uint16_t* __restrict__ bias,
                                                          uint16_t* __restrict__ y, int D, int T, int ksteps, float eps) {
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    float f[MMI_NORM_MAXP][8];
    float s1 = 0.f;
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
        const long at = mmi_xp_index(T, b, i, ksteps);
        u32x4 v = *reinterpret_cast<const u32x4*>(x + at);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f[j][2 * q] = mmi_bf16_to_f32((uint16_t)(v[q] & 0xffffu));
            f[j][2 * q + 1] = mmi_bf16_to_f32((uint16_t)(v[q] >> 16));
        }
        if (P > 0) {
            float u[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) u[e] = 0.f;
            for (int p = 0; p < P; ++p) {
                const float* pp = partial + ((long)p * B + b) * D + i;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(pp), hi = *reinterpret_cast<const f32x4*>(pp + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { u[e] += lo[e]; u[4 + e] += hi[e]; }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) f[j][e] = mmi_round_bf16(mmi_round_bf16(u[e]) + f[j][e]);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = mmi_pack_bf16x2(f[j][2 * q], f[j][2 * q + 1]);
            *reinterpret_cast<u32x4*>(x + at) = v;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s1 += f[j][e];
    }
    MMI_SHARED float red[2][16];
    const int nw = (nth + 63) / 64;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s1 += mmi_shfl_xor(s1, m);
    if ((tid & 63) == 0) red[0][tid >> 6] = s1;
    __syncthreads();
    float tot = 0.f;
    for (int wv = 0; wv < nw; ++wv) tot += red[0][wv];
    const float mean = tot / (float)D;
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float dlt = f[j][e] - mean; s2 += dlt * dlt; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s2 += mmi_shfl_xor(s2, m);
    if ((tid & 63) == 0) red[1][tid >> 6] = s2;
    __syncthreads();
    float var = 0.f;
    for (int wv = 0; wv < nw; ++wv) var += red[1][wv];
    const float rstd = mmi_rsqrtf(var / (float)D + eps);
#pragma unroll
    for (int j = 0; j < MMI_NORM_MAXP; ++j) {
        const int i = (tid + j * nth) * 8;
        if (i >= D) break;
        const u32x4 wv = *reinterpret_cast<const u32x4*>(w + i), bv = *reinterpret_cast<const u32x4*>(bias + i);
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float wl = mmi_bf16_to_f32((uint16_t)(wv[q] & 0xffffu)), wh = mmi_bf16_to_f32((uint16_t)(wv[q] >> 16));
            const float bl = mmi_bf16_to_f32((uint16_t)(bv[q] & 0xffffu)), bh = mmi_bf16_to_f32((uint16_t)(bv[q] >> 16));
            o[q] = mmi_pack_bf16x2((f[j][2 * q] - mean) * rstd * wl + bl, (f[j][2 * q + 1] - mean) * rstd * wh + bh);
        }
        *reinterpret_cast<u32x4*>(y + mmi_xp_index(T, b, i, ksteps)) = o;
    }
}

// rows of a row-major bf16 matrix [n][D] -> packed activation operand (columns col0 .. col0 + n of the source become the
// GEMM's batch rows 0 .. n): used once per stream to run the cross-attention source through the key / value projection
__global__ void k_pack_rows(const uint16_t* __restrict__ src, int n, int D, uint16_t* __restrict__ xp, int T, int ksteps) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= n * D) return;
    const int r = idx / D, k = idx - r * D;
    xp[mmi_xp_index(T, r, k, ksteps)] = src[idx];
}

// packed activation operand -> row-major rows [B][D] (the parity tap of the residual stream, mmi_lm_set_hidden_taps)
// debug trace (MMI_DEBUG_TRACE): order-independent 64-bit checksum of a buffer (sum of its 32-bit words, tail bytes included)
__global__ void k_checksum(const uint8_t* __restrict__ p, long nbytes, unsigned long long* __restrict__ out) {
    const long nwords = nbytes >> 2;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
    unsigned long long acc = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (long)gridDim.x * blockDim.x)
        acc += (unsigned long long)w[i] * (unsigned long long)(2 * (i % 1021) + 1);       // position-weighted: a swap of two words shows
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long i = nwords << 2; i < nbytes; ++i) acc += (unsigned long long)p[i] << (8 * (i & 3));
    atomicAdd(out, acc);
}

// parity tap: the int8 operand Xq[mt][kp][lane][16] (k_quant_rows_i8 / the norm kernel) -> row-major codes [B][D]
__global__ void k_unpack_q8(const uint8_t* __restrict__ xq, int B, int D, int8_t* __restrict__ dst, int T, int ksteps) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= B * D) return;
    const int r = idx / D, k = idx - r * D;
    const long at = mmi_xp_index(T, r, k, ksteps);
    const long frag = at >> 9;
    const int ln = (int)((at >> 3) & 63);
    const long mt = frag / ksteps;
    const int ks = (int)(frag - mt * ksteps);
    dst[idx] = (int8_t)xq[((mt * (ksteps >> 1) + (ks >> 1)) * 64 + ln) * 16 + (ks & 1) * 8 + (at & 7)];
}
__global__ void k_unpack_rows(const uint16_t* __restrict__ xp, int B, int D, uint16_t* __restrict__ dst, int T, int ksteps) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= B * D) return;
    const int r = idx / D, k = idx - r * D;
    dst[idx] = xp[mmi_xp_index(T, r, k, ksteps)];
}

// Cross-attention of the one new query per (model row, head) over the row's own len[b] projected condition positions
// (transformer.py:544-552, 584: no mask, no rope; keys / values change only with mmi_lm_set_row_condition).  kv: [rows][cap][2 * H *
// Dh] bf16 (keys, then values, as the in_proj's rows dim.. produce them), cap = the stream's capacity in positions; q: [rows][H *
// Dh] bf16.  One wave per (row, head); lane (r, c) = position slot r x 16-byte chunk c of the head; online softmax per slot,
// slots merged at the end.  len[b] is the same for the whole wave (one scalar load, no divergence on it); positions >= len[b]
// are never read, so what an earlier owner of the row left there does not matter.  1 <= len[b] <= cap.
struct CrossAttnArgs {
    const uint16_t* q;
    const uint16_t* kv;
    uint16_t* out;          // packed (T, out_ksteps) operand of the cross out_proj, feature = h*Dh + d
    const int* len;         // [B] live positions per model row
    int B, H, Dh, cap;
    int T, out_ksteps;
};

__global__ __launch_bounds__(64) void k_lm_cross_attn(CrossAttnArgs a) {
    const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
    const int lane = (int)threadIdx.x;
    const int Dh = a.Dh, HD = a.H * Dh, NC = Dh >> 3;          // NC in {1, 2, 4, 8, 16}
    const int RP = 64 / NC;                                     // position slots per pass
    const int r = lane / NC, c = lane - r * NC;
    const u32x4 qv = *reinterpret_cast<const u32x4*>(a.q + (long)b * HD + h * Dh + 8 * c);
    float qf[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { qf[2 * e] = __builtin_bit_cast(float, qv[e] << 16); qf[2 * e + 1] = __builtin_bit_cast(float, qv[e] & 0xffff0000u); }
    const float scale = 1.0f / sqrtf((float)Dh);
    float m_run = -INFINITY, l_run = 0.f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const int L = a.len[b];
    for (int t0 = 0; t0 < L; t0 += RP) {
        const int t = t0 + r;
        const bool live = t < L;
        const uint16_t* row = a.kv + ((long)b * a.cap + (live ? t : L - 1)) * 2 * HD + h * Dh + 8 * c;
        const u32x4 kv = *reinterpret_cast<const u32x4*>(row), vv = *reinterpret_cast<const u32x4*>(row + HD);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            d += qf[2 * e] * __builtin_bit_cast(float, kv[e] << 16);
            d += qf[2 * e + 1] * __builtin_bit_cast(float, kv[e] & 0xffff0000u);
        }
        for (int m = 1; m < NC; m <<= 1) d += mmi_shfl_xor(d, m);
        const float sc = live ? d * scale : -INFINITY;
        const float m_new = fmaxf(m_run, sc);
        const float resc = m_run == -INFINITY ? 0.f : expf(m_run - m_new);
        const float p = live ? expf(sc - m_new) : 0.f;
        l_run = l_run * resc + p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[2 * e] = acc[2 * e] * resc + p * __builtin_bit_cast(float, vv[e] << 16);
            acc[2 * e + 1] = acc[2 * e + 1] * resc + p * __builtin_bit_cast(float, vv[e] & 0xffff0000u);
        }
        m_run = m_new;
    }
    // merge the RP slots (lanes that share c): butterflies over the slot bits
    for (int m = NC; m < 64; m <<= 1) {
        const float mo = mmi_shfl_xor(m_run, m), lo = mmi_shfl_xor(l_run, m);
        const float mn = fmaxf(m_run, mo);
        const float sa = m_run == -INFINITY ? 0.f : expf(m_run - mn), sb = mo == -INFINITY ? 0.f : expf(mo - mn);
        l_run = l_run * sa + lo * sb;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = acc[e] * sa + mmi_shfl_xor(acc[e], m) * sb;
        m_run = mn;
    }
    if (r == 0) {
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = mmi_pack_bf16x2(acc[2 * e] / l_run, acc[2 * e + 1] / l_run);
        *reinterpret_cast<u32x4*>(a.out + mmi_xp_index(a.T, b, h * Dh + 8 * c, a.out_ksteps)) = ov;
    }
}

// ------------------------------------------------------------------------------------------------
// input embedding sum (lm.py:388-397): ((emb0[t1] + emb1[t2]) + ...) + text_emb[t0], each add rounded to bf16
// ------------------------------------------------------------------------------------------------
// cond: the fuser's summed condition [rows][D] (lm.py:399-400: input_ = input_ + sum_condition), or null
__global__ void k_lm_embed(const int* __restrict__ tokens, int n_codebooks, const uint16_t* __restrict__ emb,
                           int card1, const uint16_t* __restrict__ text_emb, uint16_t* __restrict__ x, int D, int T,
                           int ksteps, const uint16_t* __restrict__ cond) {
    const int b = blockIdx.y;
    const int d = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (d >= D) return;
    const int* tk = tokens + (long)b * n_codebooks;
    float acc = 0.f;
    for (int c = 1; c < n_codebooks; ++c) {
        int t = tk[c];
        float v = 0.f;
        if (t != -1) v = mmi_bf16_to_f32(emb[((long)(c - 1) * card1 + (t < 0 ? 0 : t)) * D + d]);
        acc = c == 1 ? v : mmi_round_bf16(acc + v);
    }
    int t0 = tk[0];
    float tv = 0.f;
    if (t0 != -1) tv = mmi_bf16_to_f32(text_emb[(long)(t0 < 0 ? 0 : t0) * D + d]);
    acc = n_codebooks > 1 ? mmi_round_bf16(acc + tv) : tv;
    if (cond) acc = acc + mmi_bf16_to_f32(cond[(long)b * D + d]);
    x[mmi_xp_index(T, b, d, ksteps)] = mmi_f32_to_bf16(acc);
}

// The same sum for a model whose text stream is demuxed (demux_second_text_stream, lm_utils.py:95-116): text token t is the pair
// (t % N, t / N - 1), N = text_card + 1, and embeds as bf16(T1[first] + T2[second]) (second < 0: T1[first] alone), where
// T1 = out1(E) and T2 = out2(E) were expanded at load (k_expand_emb).  t == -1 is the zero row; a second index beyond the table
// (a muxed token above N * N - 1) reads its last row.
__global__ void k_lm_embed_demux(const int* __restrict__ tokens, int n_codebooks, const uint16_t* __restrict__ emb,
                                 int card1, const uint16_t* __restrict__ text_t1, const uint16_t* __restrict__ text_t2, int N,
                                 uint16_t* __restrict__ x, int D, int T, int ksteps, const uint16_t* __restrict__ cond) {
    const int b = blockIdx.y;
    const int d = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (d >= D) return;
    const int* tk = tokens + (long)b * n_codebooks;
    float acc = 0.f;
    for (int c = 1; c < n_codebooks; ++c) {
        int t = tk[c];
        float v = 0.f;
        if (t != -1) v = mmi_bf16_to_f32(emb[((long)(c - 1) * card1 + (t < 0 ? 0 : t)) * D + d]);
        acc = c == 1 ? v : mmi_round_bf16(acc + v);
    }
    int t0 = tk[0];
    float tv = 0.f;
    if (t0 != -1) {
        const int t = t0 < 0 ? 0 : t0;
        int second = t / N - 1;
        if (second > N - 1) second = N - 1;
        tv = mmi_bf16_to_f32(text_t1[(long)(t % N) * D + d]);
        if (second >= 0) tv = mmi_round_bf16(tv + mmi_bf16_to_f32(text_t2[(long)second * D + d]));
    }
    acc = n_codebooks > 1 ? mmi_round_bf16(acc + tv) : tv;
    if (cond) acc = acc + mmi_bf16_to_f32(cond[(long)b * D + d]);
    x[mmi_xp_index(T, b, d, ksteps)] = mmi_f32_to_bf16(acc);
}

// Load time: out[v][j] = bf16(sum_i E[v][i] * W[j][i]) for E [V][R], W [D][R] (nn.Linear(R, D) applied to every row of an
// embedding table: the low-rank projection, lm_utils.py:117-124, or a demux stream's out1 / out2, :106-116), fp32 sums in i order.
// grid (cdiv(D, 256), V), 256 threads.
__global__ void k_expand_emb(const uint16_t* __restrict__ E, int R, const uint16_t* __restrict__ W, int D, uint16_t* __restrict__ out) {
    const int v = blockIdx.y;
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= D) return;
    const uint16_t* e = E + (long)v * R;
    const uint16_t* w = W + (long)j * R;
    float acc = 0.f;
    for (int i = 0; i < R; ++i) acc += mmi_bf16_to_f32(e[i]) * mmi_bf16_to_f32(w[i]);
    out[(long)v * D + j] = mmi_f32_to_bf16(acc);
}

// ------------------------------------------------------------------------------------------------
// temporal attention: RoPE + ring-KV write, split decode attention over the VALID part of the ring, combine
// ------------------------------------------------------------------------------------------------
// mmi_lm_debug_kv4_quantize: the 4-bit ring's quantiser (mmi_fp4.h) on caller-supplied bf16 blocks of 16, one thread per block -
// the conversions the in_proj epilogue runs, where a test can see them
__global__ void k_kv4_quantize(const uint16_t* __restrict__ x, long nblocks, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(x + 16 * i), hi = *reinterpret_cast<const u32x4*>(x + 16 * i + 8);
    float f[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f[2 * q] = mmi_bf16_to_f32((uint16_t)(lo[q] & 0xffffu));
        f[2 * q + 1] = mmi_bf16_to_f32((uint16_t)(lo[q] >> 16));
        f[8 + 2 * q] = mmi_bf16_to_f32((uint16_t)(hi[q] & 0xffffu));
        f[8 + 2 * q + 1] = mmi_bf16_to_f32((uint16_t)(hi[q] >> 16));
    }
    const uint32_t am0 = mmi_kv4_absmax8(f), am1 = mmi_kv4_absmax8(f + 8);
    const uint32_t sb = mmi_kv4_scale_byte(am0 > am1 ? am0 : am1);
    u32x2 c = {0u, 0u};
    if (sb) { c[0] = mmi_kv4_quant8(f, sb); c[1] = mmi_kv4_quant8(f + 8, sb); }
    *reinterpret_cast<u32x2*>(codes + 8 * i) = c;
    scales[i] = (uint8_t)sb;
}

struct LmAttnArgs {
    uint16_t* qrot;        // [B][H][Dh] roped queries (written by in_proj's epilogue)
    uint16_t* kc;          // [B][H][cap][Dh]
    uint16_t* vc;
    const long* offsets;   // [B]
    float* opart;          // [B][H][NS][Dh]
    float* ml;             // [B][H][NS][2]
    uint16_t* out;         // packed (T, out_ksteps) activations of out_proj, feature = h*Dh + d
    int B, H, Dh, cap, context, NS;
    int T, out_ksteps;
    float max_period;
    unsigned* done;        // k_lm_attn_wave with the ring split over NS workgroups: arrival counter per (session, head), 0 between launches
                           // (the last workgroup to arrive merges); null = leave the partials to k_lm_attn_combine
    int solo_rows;         // ... rings of at most this many rows are walked by workgroup y = 0 alone (the others exit at once); -1 = never
    long kv_soff;          // 4-bit ring: bytes from a codes plane (kc / vc: [B][H][cap][Dh/2]) to its scale plane ([B][H][cap][Dh/16])
};

#define MMI_ATTN_CHUNK 256
// Decode attention of the one new query per (session, head) over the VALID part of the ring only (the reference reads
// all `cap` slots through a mask, transformer.py:574-585).  grid (B*H, NS); 256 threads.  Block y walks the 256-slot
// chunks y, y+NS, ... of the ring with an online softmax; each 16-byte load covers 8 dims of one key row, DH/8 lanes share
// a row, so one wave instruction reads 64/(DH/8) consecutive rows = 1 KiB contiguous.  NS == 1 (enough (b,h) pairs to
// fill the chip): the normalised output goes straight to out_proj's packed input; otherwise partials for the combine.
// KV8: the ring holds e4m3 bytes (fp8 KV cache): a 16-byte load then covers 16 dims, DH/16 lanes share a row and one wave
// instruction reads twice as many rows; the values are widened exactly (v_cvt_pk_f32_fp8) and everything else is unchanged.
// KVF = 2: the 4-bit ring (mmi_fp4.h): a 16-byte load covers 32 dims = two blocks, and a 2-byte load beside it their two
// scale bytes; DH/32 lanes share a row; widened exactly (v_cvt_scalef32_pk_f32_fp4), scores, softmax and P.V stay fp32.
// No load reaches a slot past the valid length (every one is clamped to L - 1; the clamped re-reads carry p = 0): the result does not
// depend on what a never-written slot holds.  A slot that is written but masked by the window is used as 0 * v and needs a finite v.
template <int DH, int KVF = 0>
__global__ __launch_bounds__(256) void k_lm_attn_split(LmAttnArgs a) {
    constexpr bool KV8 = KVF == 1, KV4 = KVF == 2;
    constexpr int EPL = KV4 ? 32 : (KV8 ? 16 : 8);  // elements per lane (16 bytes)
    constexpr int ROWB = KV4 ? DH / 2 : (KV8 ? DH : 2 * DH);    // bytes per ring row
    constexpr int LPR = DH / EPL;      // lanes per row
    constexpr int RPW = 64 / LPR;      // rows per wave instruction
    constexpr int CH = MMI_ATTN_CHUNK;
    // (a mirrored session order - every second group of 8 sessions walked backwards, for load balance across CUs under a linear
    // stagger of ring depths - measured neutral, round 2: not built in)
    const int bh = blockIdx.x;
    const int b = bh / a.H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long off = a.offsets[b];
    const long end_new = off + 1;
    const int end_index = (int)(off % a.cap);
    const int L = (int)(end_new < (long)a.cap ? end_new : (long)a.cap);
    MMI_SHARED float sc[CH];
    MMI_SHARED float wred[8];
    MMI_SHARED float ored[4 * DH];
    const int seg = lane % LPR, rsub = lane / LPR;
    float qv[EPL];
#pragma unroll
    for (int v = 0; v < EPL / 8; ++v) {
        u32x4 qq = *reinterpret_cast<const u32x4*>(a.qrot + (long)bh * DH + seg * EPL + v * 8);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            qv[v * 8 + 2 * q] = mmi_bf16_to_f32((uint16_t)(qq[q] & 0xffffu));
            qv[v * 8 + 2 * q + 1] = mmi_bf16_to_f32((uint16_t)(qq[q] >> 16));
        }
    }
    // 16 bytes of a ring row -> EPL fp32 values (sc2: the two scale bytes of a 4-bit lane's blocks)
    auto widen = [](const u32x4& r, uint32_t sc2, float* f) {
        if constexpr (KV4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) mmi_kv4_widen8(r[q], (sc2 >> (8 * (q >> 1))) & 0xffu, f + 8 * q);
        } else if constexpr (KV8) {
#pragma unroll
            for (int q = 0; q < 4; ++q) mmi_fp8x4_to_f32(r[q], f + 4 * q);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f[2 * q] = mmi_bf16_to_f32((uint16_t)(r[q] & 0xffffu));
                f[2 * q + 1] = mmi_bf16_to_f32((uint16_t)(r[q] >> 16));
            }
        }
    };
    const uint8_t* kbase = reinterpret_cast<const uint8_t*>(a.kc) + (long)bh * a.cap * ROWB;
    const uint8_t* vbase = reinterpret_cast<const uint8_t*>(a.vc) + (long)bh * a.cap * ROWB;
    // 4-bit ring: the scale planes, DH / 16 bytes per row, two per lane
    const uint8_t* ksbase = reinterpret_cast<const uint8_t*>(a.kc) + a.kv_soff + (long)bh * a.cap * (DH / 16);
    const uint8_t* vsbase = reinterpret_cast<const uint8_t*>(a.vc) + a.kv_soff + (long)bh * a.cap * (DH / 16);
    const float scale = 1.0f / sqrtf((float)DH);
    constexpr int PER_WAVE = CH / 4;
    float m_run = -INFINITY, l_run = 0.f;
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int c0 = (int)blockIdx.y * CH; c0 < L; c0 += (int)gridDim.y * CH) {     // block-uniform trip count
        // ---- scores of this chunk: all of the wave's key rows are requested up front (unconditional loads from a clamped
        // slot; a load under `if (valid)` would be serialised behind s_waitcnt vmcnt(0)), then reduced
        constexpr int NIT = PER_WAVE / RPW;
        constexpr int NB = NIT < 8 ? NIT : 8;             // rows in flight per lane: 8 x 16 bytes keeps the kernel at <= 96 VGPRs
#pragma unroll 1
        for (int h0 = 0; h0 < NIT; h0 += NB) {
            u32x4 kk[NB];
            uint32_t ks[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int slot = min(c0 + wave * PER_WAVE + (h0 + i) * RPW + rsub, L - 1);
                kk[i] = *reinterpret_cast<const u32x4*>(kbase + (long)slot * ROWB + seg * 16);
                if constexpr (KV4) ks[i] = *reinterpret_cast<const uint16_t*>(ksbase + (long)slot * (DH / 16) + seg * 2);
                else ks[i] = 0u;
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int rl = wave * PER_WAVE + (h0 + i) * RPW + rsub;
                const int slot = c0 + rl;
                bool valid = slot < L;
                if (valid) {   // absolute position of the slot (transformer.py:258-286) and the causal/context mask (:574-582)
                    int delta = slot - end_index;
                    long pos = delta <= 0 ? off + delta : off + delta - a.cap;
                    long dq = off - pos;
                    valid = pos >= 0 && dq >= 0 && dq < a.context;
                }
                float dot = 0.f;
                float kf[EPL];
                widen(kk[i], ks[i], kf);
#pragma unroll
                for (int e = 0; e < EPL; ++e) dot += qv[e] * kf[e];
#pragma unroll
                for (int m = LPR / 2; m >= 1; m >>= 1) dot += mmi_shfl_xor(dot, m);
                if (seg == 0) sc[rl] = valid ? dot * scale : -INFINITY;
            }
        }
        __syncthreads();
        // ---- online softmax update
        const float sv = sc[tid];
        float mx = sv;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, mmi_shfl_xor(mx, m));
        if (lane == 0) wred[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
        const float m_new = fmaxf(m_run, mx);
        const float p = (m_new == -INFINITY) ? 0.f : expf(sv - m_new);
        float sum = p;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sum += mmi_shfl_xor(sum, m);
        if (lane == 0) wred[4 + wave] = sum;
        sc[tid] = p;
        __syncthreads();
        sum = (wred[4] + wred[5]) + (wred[6] + wred[7]);
        const float resc = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);
        l_run = l_run * resc + sum;
        m_run = m_new;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] *= resc;
        // ---- P.V (value rows requested up front as well, clamped to L - 1 like the keys: the re-read rows past L carry p = 0)
#pragma unroll 1
        for (int h0 = 0; h0 < NIT; h0 += NB) {
            u32x4 vv[NB];
            uint32_t vs[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int slot = min(c0 + wave * PER_WAVE + (h0 + i) * RPW + rsub, L - 1);
                vv[i] = *reinterpret_cast<const u32x4*>(vbase + (long)slot * ROWB + seg * 16);
                if constexpr (KV4) vs[i] = *reinterpret_cast<const uint16_t*>(vsbase + (long)slot * (DH / 16) + seg * 2);
                else vs[i] = 0u;
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int rl = wave * PER_WAVE + (h0 + i) * RPW + rsub;
                const float pr = (c0 + rl < L) ? sc[rl] : 0.f;
                float vf[EPL];
                widen(vv[i], vs[i], vf);
#pragma unroll
                for (int e = 0; e < EPL; ++e) acc[e] += pr * vf[e];
            }
        }
        __syncthreads();     // sc / wred are rewritten by the next chunk
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e)
#pragma unroll
        for (int m = 32; m >= LPR; m >>= 1) acc[e] += mmi_shfl_xor(acc[e], m);
    if (rsub == 0) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) ored[wave * DH + seg * EPL + e] = acc[e];
    }
    __syncthreads();
    if (tid < DH) {
        const float o = (ored[tid] + ored[DH + tid]) + (ored[2 * DH + tid] + ored[3 * DH + tid]);
        if (gridDim.y == 1) {
            a.out[mmi_xp_index(a.T, b, (bh % a.H) * DH + tid, a.out_ksteps)] = mmi_f32_to_bf16(o / l_run);
        } else {
            a.opart[((long)bh * gridDim.y + blockIdx.y) * DH + tid] = o;
        }
    }
    if (gridDim.y > 1 && tid == 0) {
        float* mlp = a.ml + ((long)bh * gridDim.y + blockIdx.y) * 2;
        mlp[0] = m_run;
        mlp[1] = l_run;
    }
}

// The same attention with ONE online softmax per lane group and no workgroup barrier inside the loop (round 4).  k_lm_attn_split
// walks a 256-row chunk in four dependent memory round trips (keys x 2, softmax through LDS, values x 2) with three barriers
// in between, and all of a CU's co-resident workgroups do so in lockstep: at the benchmark's ring depths (150 ... 550 rows per
// head) the kernel is bound by those round trips, not by HBM (23 us for 78 MB).  Here the ring's rows are dealt out in
// row groups (one wave instruction = RPW consecutive rows = 1 KiB) round-robin over ALL waves that serve the (session, head)
// pair - 4 per workgroup x gridDim.y workgroups - and every wave keeps, per row slot (the lanes that share `rsub`), its own
// running (max, sum, accumulator): a round requests NB key groups AND their NB value groups at once (the values do not depend
// on the scores), the next round's 2 NB loads are issued before this round's arithmetic, and nothing but registers and
// cross-lane shuffles is touched until the slots and the waves are merged once at the end.
// KVF: the ring form, as for k_lm_attn_split (1 = e4m3, 2 = E2M1 under block scales: a 2-byte scale load beside each 16-byte load).
// The 16-byte key and value loads are non-temporal, like every weight stream of the step: a ring row is read by exactly one wave
// instruction of one workgroup per launch and by nobody else before the next frame, so it need not displace what the caches hold
// (-0.07 .. -0.09 ms per flagship step, -0.4 ms on full rings; profiles/attn_ramp/README.md).  The query, the offsets, the 4-bit ring's
// 2-byte scale loads and every store keep the default policy.
#define MMI_AW_LD16(p) mmi_load_nt(reinterpret_cast<const u32x4*>(p))
#ifndef MMI_ATTN_STAMP
#define MMI_ATTN_STAMP(i, dep)       // scripts/attn_stamps.hip defines these three: device-clock stamps at the kernel's stages
#define MMI_ATTN_STAMP_LANDED(i, first)
#define MMI_ATTN_STAMP_STORED(i)
#endif
template <int DH, int KVF = 0>
__global__ __launch_bounds__(256, KVF ? 2 : 4) void k_lm_attn_wave(LmAttnArgs a) {      // bf16 ring: <= 128 VGPRs, 4 workgroups per CU
    constexpr bool KV8 = KVF == 1, KV4 = KVF == 2;
    constexpr int EPL = KV4 ? 32 : (KV8 ? 16 : 8);  // elements per lane (16 bytes)
    constexpr int ROWB = KV4 ? DH / 2 : (KV8 ? DH : 2 * DH);    // bytes per ring row
    constexpr int LPR = DH / EPL;      // lanes per row
    constexpr int RPW = 64 / LPR;      // rows per wave instruction
    constexpr int NB = KV4 ? 2 : 4;    // row groups per round (x 2 buffers x (key + value) = 16 loads of 16 bytes in flight per lane; the 4-bit
                                       // ring, 32 accumulators and 32 query elements per lane, keeps half as many: no scratch at head dim 128)
    const int bh = blockIdx.x;
    const int b = bh / a.H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long off = a.offsets[b];
    const int end_index = (int)(off % a.cap);
    const long end_new = off + 1;
    const int L = (int)(end_new < (long)a.cap ? end_new : (long)a.cap);
    const int seg = lane % LPR, rsub = lane / LPR;
    float qv[EPL];
    u32x4 qp = {0u, 0u, 0u, 0u};      // bf16 ring: the lane's 8 query elements stay packed (v_dot2c_f32_bf16 takes both operands packed)
#pragma unroll
    for (int v = 0; v < EPL / 8; ++v) {
        u32x4 qq = *reinterpret_cast<const u32x4*>(a.qrot + (long)bh * DH + seg * EPL + v * 8);
        if (v == 0) qp = qq;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            qv[v * 8 + 2 * q] = mmi_bf16_to_f32((uint16_t)(qq[q] & 0xffffu));
            qv[v * 8 + 2 * q + 1] = mmi_bf16_to_f32((uint16_t)(qq[q] >> 16));
        }
    }
    auto widen = [](const u32x4& r, uint32_t sc2, float* f) {
        if constexpr (KV4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) mmi_kv4_widen8(r[q], (sc2 >> (8 * (q >> 1))) & 0xffu, f + 8 * q);
        } else if constexpr (KV8) {
#pragma unroll
            for (int q = 0; q < 4; ++q) mmi_fp8x4_to_f32(r[q], f + 4 * q);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f[2 * q] = mmi_bf16_to_f32((uint16_t)(r[q] & 0xffffu));
                f[2 * q + 1] = mmi_bf16_to_f32((uint16_t)(r[q] >> 16));
            }
        }
    };
    // wave-uniform base (scalar registers) + a 32-bit lane offset: the loads take the saddr form, no 64-bit address per lane
    const uint8_t* kbase = reinterpret_cast<const uint8_t*>(a.kc) + (long)bh * a.cap * ROWB;
    const uint8_t* vbase = reinterpret_cast<const uint8_t*>(a.vc) + (long)bh * a.cap * ROWB;
    const unsigned loff = (unsigned)(seg * 16);
    // 4-bit ring: the scale planes (DH / 16 bytes per row, two per lane), wave-uniform bases as well
    const uint8_t* ksbase = reinterpret_cast<const uint8_t*>(a.kc) + a.kv_soff + (long)bh * a.cap * (DH / 16);
    const uint8_t* vsbase = reinterpret_cast<const uint8_t*>(a.vc) + a.kv_soff + (long)bh * a.cap * (DH / 16);
    const unsigned lsoff = (unsigned)(seg * 2);
    const float scale = 1.0f / sqrtf((float)DH);
    // One workgroup per (session, head) (gridDim.y == 1: which wave walks which row group does not depend on the ring depth): the
    // FIRST round's keys and values are requested before the session's offset - a cold scalar load of its own, ~1 us into a
    // ~40 us launch - has come back: row groups wave, wave + 4, ... of the ring's first slots, any of which lies inside the
    // allocation; rows past the valid part are masked where they are used (slot < L), as the clamped re-reads always were, and
    // their values are zeroed below once L is known
    u32x4 kA[NB], vA[NB], kB[NB], vB[NB];
    uint32_t ksA[NB], vsA[NB], ksB[NB], vsB[NB];      // 4-bit ring only: the rows' scale byte pairs
#pragma unroll
    for (int i = 0; i < NB; ++i) ksA[i] = vsA[i] = ksB[i] = vsB[i] = 0u;
    const bool early = gridDim.y == 1;
    MMI_ATTN_STAMP(0, loff)
    if (early) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int slot_ = min((wave + i * 4) * RPW + rsub, a.cap - 1);
            const unsigned o_ = (unsigned)slot_ * (unsigned)ROWB + loff;
            kA[i] = MMI_AW_LD16(kbase + o_);
            vA[i] = MMI_AW_LD16(vbase + o_);
            if constexpr (KV4) {
                const unsigned so_ = (unsigned)slot_ * (unsigned)(DH / 16) + lsoff;
                ksA[i] = *reinterpret_cast<const uint16_t*>(ksbase + so_);
                vsA[i] = *reinterpret_cast<const uint16_t*>(vsbase + so_);
            }
        }
    }
    // The early loads came from slots up to cap - 1, whatever the ring holds there.  A slot that was never written (>= L) is used as
    // p * v with p = 0, which is 0 only for a finite v: once per launch - not per round - such a value row reads as zeros (4-bit
    // ring: scale byte 0 = the factor 0), so the result does not depend on what an unwritten slot holds (its key only feeds a score
    // that the mask replaces).  Every later load is clamped to L - 1.
    MMI_ATTN_STAMP(1, L)
    if (early) {
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if ((wave + i * 4) * RPW + rsub >= L) { vA[i] = u32x4{0u, 0u, 0u, 0u}; vsA[i] = 0u; }
    }
    // context >= capacity (the LM's ring: both 3000): every written slot is inside the window - slot s < L holds a position p with
    // 0 <= offset - p < cap - so the mask (transformer.py:574-582) reduces to `slot < L` and the per-row position arithmetic is
    // skipped (wave-uniform branch); a ring longer than its attention window keeps it
    const bool windowed = a.context < a.cap;
    // Fewer (session, head) pairs than it takes to fill the chip (one real-time session: 32): the ring is shared out over gridDim.y
    // workgroups - but only where it is long enough to be worth the merge: a short ring is walked by workgroup y = 0 alone, which
    // then writes the final output itself (no partials, no fence, and no combine launch either way: see the end of the kernel)
    const bool solo = (int)gridDim.y > 1 && L <= a.solo_rows;
    if (solo && blockIdx.y != 0) return;
    const int nsplit = solo ? 1 : (int)gridDim.y;
    const int total = nsplit * 4, wg = (solo ? 0 : (int)blockIdx.y * 4) + wave;  // waves serving this pair, and which one this is
    const int ngroups = (L + RPW - 1) / RPW;
    const int nmine = wg < ngroups ? (ngroups - wg + total - 1) / total : 0;       // row groups wg, wg + total, ...
    const int nrounds = (nmine + NB - 1) / NB;
    float m_run = -INFINITY, l_run = 0.f, acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    // every load is unconditional from a clamped (valid) slot - a load under a branch would be serialised behind
    // s_waitcnt vmcnt(0) - and rows past the end carry probability 0
#define MMI_AW_LOAD(KK, VV, KS, VS, j0)                                                          \
    _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                            \
        const int slot_ = min((wg + ((j0) + i) * total) * RPW + rsub, L - 1);                   \
        const unsigned o_ = (unsigned)slot_ * (unsigned)ROWB + loff;                            \
        KK[i] = MMI_AW_LD16(kbase + o_);                                                        \
        VV[i] = MMI_AW_LD16(vbase + o_);                                                        \
        if constexpr (KV4) {                                                                     \
            const unsigned so_ = (unsigned)slot_ * (unsigned)(DH / 16) + lsoff;                 \
            KS[i] = *reinterpret_cast<const uint16_t*>(ksbase + so_);                           \
            VS[i] = *reinterpret_cast<const uint16_t*>(vsbase + so_);                           \
        }                                                                                        \
    }
#define MMI_AW_USE(KK, VV, KS, VS, j0)                                                                 \
    {                                                                                            \
        float s_[NB];                                                                            \
        float mx_ = -INFINITY;                                                                   \
        _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                        \
            const int j_ = (j0) + i;                                                             \
            const int slot_ = (wg + j_ * total) * RPW + rsub;                                    \
            bool valid_ = j_ < nmine && slot_ < L;                                               \
            if (windowed && valid_) {   /* absolute position of the slot (transformer.py:258-286), causal / context mask (:574-582) */ \
                const int delta_ = slot_ - end_index;                                            \
                const long pos_ = delta_ <= 0 ? off + delta_ : off + delta_ - a.cap;             \
                const long dq_ = off - pos_;                                                     \
                valid_ = pos_ >= 0 && dq_ >= 0 && dq_ < a.context;                               \
            }                                                                                    \
            float dot_ = 0.f;                                                                    \
            if constexpr (KVF != 0) {                                                            \
                float kf_[EPL];                                                                  \
                widen(KK[i], KS[i], kf_);                                                              \
                _Pragma("unroll") for (int e = 0; e < EPL; ++e) dot_ = mmi_fma(qv[e], kf_[e], dot_); \
            } else {                    /* 4 packed-pair dot products instead of 8 unpacks + 8 FMAs */ \
                _Pragma("unroll") for (int q = 0; q < 4; ++q) dot_ = mmi_dot2_bf16(KK[i][q], qp[q], dot_); \
            }                                                                                    \
            dot_ = mmi_group_sum<LPR>(dot_);                /* DPP row operations, no trip through the LDS crossbar */ \
            s_[i] = valid_ ? dot_ * scale : -INFINITY;                                           \
            mx_ = fmaxf(mx_, s_[i]);                                                             \
        }                                                                                        \
        const float m_new_ = fmaxf(m_run, mx_);                                                  \
        if (m_new_ != -INFINITY) {                                                               \
            const float resc_ = m_run == -INFINITY ? 0.f : expf(m_run - m_new_);                 \
            l_run *= resc_;                                                                      \
            _Pragma("unroll") for (int e = 0; e < EPL; ++e) acc[e] *= resc_;                    \
            _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                    \
                const float p_ = expf(s_[i] - m_new_);        /* exp(-inf) = 0 for masked rows */ \
                l_run += p_;                                                                     \
                if constexpr (KVF != 0) {                                                        \
                    float vf_[EPL];                                                              \
                    widen(VV[i], VS[i], vf_);                                                         \
                    _Pragma("unroll") for (int e = 0; e < EPL; ++e) acc[e] = mmi_fma(p_, vf_[e], acc[e]); \
                } else {                /* packed FMAs: two accumulator elements per instruction */ \
                    const f32x2 pp_ = {p_, p_};                                                  \
                    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                             \
                        const f32x2 v2_ = {__builtin_bit_cast(float, VV[i][q] << 16), __builtin_bit_cast(float, VV[i][q] & 0xffff0000u)}; \
                        const f32x2 a2_ = mmi_pk_fma(pp_, v2_, f32x2{acc[2 * q], acc[2 * q + 1]}); \
                        acc[2 * q] = a2_[0];                                                     \
                        acc[2 * q + 1] = a2_[1];                                                 \
                    }                                                                            \
                }                                                                                \
            }                                                                                    \
            m_run = m_new_;                                                                      \
        }                                                                                        \
    }
    if (nrounds > 0) {
        if (!early) { MMI_AW_LOAD(kA, vA, ksA, vsA, 0) }
        for (int r = 0; r < nrounds; r += 2) {
            MMI_AW_LOAD(kB, vB, ksB, vsB, (r + 1) * NB)          // clamped past the end: re-reads the last row (cache hit), masked on use
            MMI_ATTN_STAMP_LANDED(2, r == 0)
            MMI_AW_USE(kA, vA, ksA, vsA, r * NB)
            MMI_AW_LOAD(kA, vA, ksA, vsA, (r + 2) * NB)
            MMI_AW_USE(kB, vB, ksB, vsB, (r + 1) * NB)
        }
    }
    MMI_ATTN_STAMP(3, l_run)
#undef MMI_AW_LOAD
#undef MMI_AW_USE
#undef MMI_AW_LD16
    // ---- merge the RPW row slots of the wave (lanes that share `seg`): butterflies over the slot bits
#pragma unroll
    for (int mk = LPR; mk < 64; mk <<= 1) {
        const float mo = mmi_shfl_xor(m_run, mk), lo = mmi_shfl_xor(l_run, mk);
        const float mn = fmaxf(m_run, mo);
        const float sa = m_run == -INFINITY ? 0.f : expf(m_run - mn), sb = mo == -INFINITY ? 0.f : expf(mo - mn);
        l_run = l_run * sa + lo * sb;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = acc[e] * sa + mmi_shfl_xor(acc[e], mk) * sb;
        m_run = mn;
    }
    MMI_ATTN_STAMP(4, l_run)
    // ---- merge the 4 waves through LDS (the only barrier of the kernel)
    MMI_SHARED float wm[4], wl[4];
    MMI_SHARED float wacc[4 * DH];
    if (rsub == 0) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) wacc[wave * DH + seg * EPL + e] = acc[e];
        if (seg == 0) { wm[wave] = m_run; wl[wave] = l_run; }
    }
    __syncthreads();
    if (tid < DH) {
        const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float sw = wm[w] == -INFINITY ? 0.f : expf(wm[w] - M);
            num += sw * wacc[w * DH + tid];
            den += sw * wl[w];
        }
        MMI_ATTN_STAMP(5, num)
        if (nsplit == 1) {
            a.out[mmi_xp_index(a.T, b, (bh % a.H) * DH + tid, a.out_ksteps)] = mmi_f32_to_bf16(num / den);
            MMI_ATTN_STAMP_STORED(6)
        } else {
            a.opart[((long)bh * gridDim.y + blockIdx.y) * DH + tid] = num;
            if (tid == 0) {
                float* mlp = a.ml + ((long)bh * gridDim.y + blockIdx.y) * 2;
                mlp[0] = M;
                mlp[1] = den;
            }
        }
    }
    if (nsplit == 1 || a.done == nullptr) return;        // (no counter: k_lm_attn_combine follows in a launch of its own)
    // ---- the workgroup that arrives LAST merges the partials: out = sum_c e^{m_c - M} O_c / sum_c e^{m_c - M} l_c.  The safety net
    // of the engine's shallow-ring program (lm_engine.hip attn_variant), which has no merge launch: the release + arrival + acquire
    // chain costs about 8 us per layer more than that launch would, so rings the host KNOWS may be deep take the other program
    MMI_SHARED unsigned s_last;
    __syncthreads();                                     // the partials of this workgroup are stored
    if (tid == 0) {
        const unsigned seen = mmi_arrive_release(a.done + bh);
        s_last = seen == (unsigned)gridDim.y - 1u ? 1u : 0u;
        if (s_last) {
            mmi_store_relaxed_agent(a.done + bh, 0u);    // everyone has arrived: the counter is ready for the next launch
            mmi_acquire_agent();
        }
    }
    __syncthreads();
    if (!s_last) return;
    if (tid < DH) {
        const int NSg = (int)gridDim.y;
        const float* ml = a.ml + (long)bh * NSg * 2;
        float M = -INFINITY;
        for (int c = 0; c < NSg; ++c) M = fmaxf(M, ml[2 * c]);
        float num = 0.f, den = 0.f;
        for (int c = 0; c < NSg; ++c) {
            const float m = ml[2 * c];
            if (m == -INFINITY) continue;
            const float w = expf(m - M);
            num += w * a.opart[((long)bh * NSg + c) * DH + tid];
            den += w * ml[2 * c + 1];
        }
        a.out[mmi_xp_index(a.T, b, (bh % a.H) * DH + tid, a.out_ksteps)] = mmi_f32_to_bf16(num / den);
    }
}

// merge the chunk partials: out = sum_c e^{m_c-M} O_c / sum_c e^{m_c-M} l_c  -> bf16 [B][H*Dh]
__global__ void k_lm_attn_combine(LmAttnArgs a) {
    const int bh = blockIdx.x;
    const int Dh = a.Dh;
    const float* ml = a.ml + (long)bh * a.NS * 2;
    float M = -INFINITY;
    for (int c = 0; c < a.NS; ++c) M = fmaxf(M, ml[2 * c]);
    for (int d = threadIdx.x; d < Dh; d += blockDim.x) {
        float num = 0.f, den = 0.f;
        for (int c = 0; c < a.NS; ++c) {
            float m = ml[2 * c];
            if (m == -INFINITY) continue;
            float w = expf(m - M);
            num += w * a.opart[((long)bh * a.NS + c) * Dh + d];
            den += w * ml[2 * c + 1];
        }
        a.out[mmi_xp_index(a.T, bh / a.H, (bh % a.H) * Dh + d, a.out_ksteps)] = mmi_f32_to_bf16(num / den);
    }
}

// ------------------------------------------------------------------------------------------------
// depformer attention: step `k` of the 8 per frame; keys 0..k of a cache that is rebuilt every frame
// (no RoPE: depformer_pos_emb "none"; KV ignores the exec mask, transformer.py:251-253,478)
// one wave per (b, head); Dh <= 64
// ------------------------------------------------------------------------------------------------
struct DepAttnArgs {
    const uint16_t* qkv;   // [B][3*H*Dh]
    uint16_t* kc;          // [B][H][steps][Dh]
    uint16_t* vc;
    uint16_t* out;         // packed (T, out_ksteps), feature = h*Dh + lane
    int B, H, Dh, steps, k;
    int T, out_ksteps;
};

// ROWS: the rows of the frame's cache held in registers, >= steps (16: up to 16 micro-steps; 32: the TTS family's 17..32)
template <int ROWS>
__global__ __launch_bounds__(64) void k_dep_attn(DepAttnArgs a) {
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const int lane = threadIdx.x, Dh = a.Dh, HD = a.H * Dh;
    const bool on = lane < Dh;
    const uint16_t* row = a.qkv + (long)b * 3 * HD;
    uint16_t* kcb = a.kc + ((long)b * a.H + h) * a.steps * Dh;
    uint16_t* vcb = a.vc + ((long)b * a.H + h) * a.steps * Dh;
    float q = 0.f;
    uint16_t kn = 0, vn = 0;
    if (on) {
        q = mmi_bf16_to_f32(row[h * Dh + lane]);
        kn = row[HD + h * Dh + lane];
        vn = row[2 * HD + h * Dh + lane];
        kcb[(long)a.k * Dh + lane] = kn;
        vcb[(long)a.k * Dh + lane] = vn;
    }
    const float scale = 1.0f / sqrtf((float)Dh);
    // rows 0..k-1 of this frame's cache, all requested up front (unconditional loads from a clamped row); steps <= ROWS
    float kr[ROWS], vr[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int jc = j < a.k ? j : (a.k > 0 ? a.k - 1 : 0);
        const int lc = on ? lane : 0;
        kr[j] = mmi_bf16_to_f32(kcb[(long)jc * Dh + lc]);
        vr[j] = mmi_bf16_to_f32(vcb[(long)jc * Dh + lc]);
    }
    float sc[ROWS];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        if (j <= a.k) {
            float kv = 0.f;
            if (on) kv = (j == a.k) ? mmi_bf16_to_f32(kn) : kr[j];
            float d = q * kv;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) d += mmi_shfl_xor(d, m);
            sc[j] = d * scale;
            mx = fmaxf(mx, sc[j]);
        }
    }
    float den = 0.f, o = 0.f;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        if (j <= a.k) {
            float p = expf(sc[j] - mx);
            den += p;
            float vv = 0.f;
            if (on) vv = (j == a.k) ? mmi_bf16_to_f32(vn) : vr[j];
            o += p * vv;
        }
    }
    if (on) a.out[mmi_xp_index(a.T, b, h * Dh + lane, a.out_ksteps)] = mmi_f32_to_bf16(o / den);
}

// The same attention for Dh a multiple of 8 (<= 64) and <= 8 positions per frame - Moshi's depth transformer - with far fewer
// dependent instructions: one wave per (session, head), lane (j, c) = position j x 16-byte chunk c of the head: it loads its
// chunk of q, of key row j and of value row j once (the newest row straight from the in_proj output, which the lanes of
// position k also copy into the frame's cache), reduces the score over the 8 chunk lanes, the softmax and P.V over the 8
// position groups (3 butterfly steps each), and the lanes of position 0 store 8 output features as one 16-byte vector.
// One (session, head) by the calling wave, in two parts so that a wave serving several pairs (k_dep_attn_out_proj) has all their
// loads in flight before the first dependent instruction.  mmi_dep_attn8_load: the lane's 16-byte chunk of q, of key row j and of
// value row j (write_cache: the lanes of position k also copy the newest key / value row into the frame's cache);
// mmi_dep_attn8_reduce: on return the lanes of position 0 (j == 0, c < Dh / 8) hold output features 8 c .. 8 c + 7 of the head as
// packed bf16.
struct DepAttnOperands { u32x4 q, k, v; };
__device__ __forceinline__ DepAttnOperands mmi_dep_attn8_load(const DepAttnArgs& a, int b, int h, int lane, bool write_cache) {
    const int Dh = a.Dh, HD = a.H * Dh, NC = Dh >> 3;
    const int j = lane >> 3, c = lane & 7;
    const int jc = j < a.k ? j : a.k, cc = c < NC ? c : 0;          // clamped: every lane loads from a valid address
    const uint16_t* row = a.qkv + (long)b * 3 * HD + h * Dh + 8 * cc;
    uint16_t* kcb = a.kc + ((long)b * a.H + h) * a.steps * Dh + 8 * cc;
    uint16_t* vcb = a.vc + ((long)b * a.H + h) * a.steps * Dh + 8 * cc;
    const bool newest = jc == a.k;
    DepAttnOperands o;
    o.q = *reinterpret_cast<const u32x4*>(row);
    o.k = *reinterpret_cast<const u32x4*>(newest ? row + HD : kcb + (long)jc * Dh);
    o.v = *reinterpret_cast<const u32x4*>(newest ? row + 2 * HD : vcb + (long)jc * Dh);
    if (write_cache && j == a.k && c < NC) {                        // this frame's cache, position k (transformer.py:243-253)
        *reinterpret_cast<u32x4*>(kcb + (long)a.k * Dh) = o.k;
        *reinterpret_cast<u32x4*>(vcb + (long)a.k * Dh) = o.v;
    }
    return o;
}
__device__ __forceinline__ u32x4 mmi_dep_attn8_reduce(const DepAttnArgs& a, const DepAttnOperands& in, int lane) {
    const int Dh = a.Dh, NC = Dh >> 3;
    const int j = lane >> 3, c = lane & 7;
    const u32x4 qv = in.q, kv = in.k, vv = in.v;
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        d += __builtin_bit_cast(float, qv[e] << 16) * __builtin_bit_cast(float, kv[e] << 16);
        d += __builtin_bit_cast(float, qv[e] & 0xffff0000u) * __builtin_bit_cast(float, kv[e] & 0xffff0000u);
    }
    if (c >= NC) d = 0.f;
    d += mmi_shfl_xor(d, 1); d += mmi_shfl_xor(d, 2); d += mmi_shfl_xor(d, 4);
    const bool live = j <= a.k;
    const float sc = live ? d * (1.0f / sqrtf((float)Dh)) : -INFINITY;
    float mx = sc;
    mx = fmaxf(mx, mmi_shfl_xor(mx, 8)); mx = fmaxf(mx, mmi_shfl_xor(mx, 16)); mx = fmaxf(mx, mmi_shfl_xor(mx, 32));
    const float p = live ? expf(sc - mx) : 0.f;
    float den = p;
    den += mmi_shfl_xor(den, 8); den += mmi_shfl_xor(den, 16); den += mmi_shfl_xor(den, 32);
    float o[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o[2 * e] = p * __builtin_bit_cast(float, vv[e] << 16);
        o[2 * e + 1] = p * __builtin_bit_cast(float, vv[e] & 0xffff0000u);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] += mmi_shfl_xor(o[e], 8); o[e] += mmi_shfl_xor(o[e], 16); o[e] += mmi_shfl_xor(o[e], 32);
    }
    u32x4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = mmi_pack_bf16x2(o[2 * e] / den, o[2 * e + 1] / den);
    return ov;
}
__device__ __forceinline__ u32x4 mmi_dep_attn8_wave(const DepAttnArgs& a, int b, int h, int lane, bool write_cache) {
    return mmi_dep_attn8_reduce(a, mmi_dep_attn8_load(a, b, h, lane, write_cache), lane);
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void k_dep_attn8(DepAttnArgs a) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int bh = (int)blockIdx.x * NW + wave;
    if (bh >= a.B * a.H) return;
    const int b = bh / a.H, h = bh - b * a.H;
    const u32x4 ov = mmi_dep_attn8_wave(a, b, h, lane, true);
    const int j = lane >> 3, c = lane & 7;
    if (j == 0 && c < (a.Dh >> 3)) *reinterpret_cast<u32x4*>(a.out + mmi_xp_index(a.T, b, h * a.Dh + 8 * c, a.out_ksteps)) = ov;
}

// The depth transformer's attention INSIDE its out_proj (one session - the engine instantiates BMAX = 1 - at the 16-row tile,
// micro-steps >= 1): the GEMM's K axis is the attention output [head][Dh], a wave's K-slice is whole heads, so every workgroup's
// wave computes the (session, head) pairs of its own slice itself - k_dep_attn8's arithmetic, straight after requesting its weight
// fragments - and hands the 8-feature pieces to the lanes that hold them in the MFMA operand through LDS: two pairs per wave, a
// few hundred bytes from L2.  What it removes is a 4.5 us launch on the depth transformer's dependent chain, 42 times per step
// (the GEMM grows by 1.6 us).  The workgroups all compute the same thing; workgroup 0 also writes the newest key / value rows to
// the frame's cache.  Bit-identical to the two launches (the same per-pair functions, the same operand values).
template <int WAVES, int HPW, int BMAX>
__global__ __launch_bounds__(WAVES * 64) void k_dep_attn_out_proj(GemmArgs a, DepAttnArgs d) {
    constexpr int TN = 16, R = 4, KPWMAX = 4;
    typedef float acc_t __attribute__((ext_vector_type(R)));
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int os = a.osplit > 1 ? a.osplit : 1;                     // octet sharing as in k_gemm_xp
    const int bx = (int)blockIdx.x / os, part = (int)blockIdx.x - bx * os;
    const int nt0 = bx;
    const int g_lo = part * ((TN / 8) / os), g_hi = os > 1 ? g_lo + (TN / 8) / os : TN / 8;
    const int ro = (lane >> 3) & (TN / 8 - 1);
    const int wlane = (ro >= g_lo && ro < g_hi) ? lane : ((lane & ~((TN / 8 - 1) << 3)) | (g_lo << 3));
    const u32x4 pre = mmi_gemm_prefetch_addend<TN, 1, 1>(a, nt0);
    const int kper = (a.KSTEPS + WAVES - 1) / WAVES;                // <= KPWMAX, kper * 32 a multiple of Dh (launcher)
    const int ks0 = min(a.KSTEPS, wave * kper);
    const int nks = min(a.KSTEPS, ks0 + kper) - ks0;
    const int last = nks > 0 ? nks - 1 : 0;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const u32x4* wp = a.wp + ((long)min(nt0, a.NT - 1) * a.KSTEPS + min(ks0, a.KSTEPS - 1)) * 64 + wlane;
    u32x4 wv[KPWMAX];
#pragma unroll
    for (int u = 0; u < KPWMAX; ++u) wv[u] = mmi_load_nt(wp + min(u, last) * 64);
    // ---- the attention of this wave's heads
    MMI_SHARED __attribute__((aligned(16))) u32x4 xs[WAVES][KPWMAX][64];
    const int h0 = ks0 * 32 / d.Dh, nh = nks * 32 / d.Dh;
    const int j = lane >> 3, c = lane & 7;
    DepAttnOperands in[HPW][BMAX];                                   // every pair's loads first (clamped pairs repeat a live one)
#pragma unroll
    for (int hh = 0; hh < HPW; ++hh)
#pragma unroll
        for (int b = 0; b < BMAX; ++b)
            in[hh][b] = mmi_dep_attn8_load(d, min(b, d.B - 1), min(h0 + hh, d.H - 1), lane, false);
    if (blockIdx.x == 0) {                                           // the newest key / value rows into the frame's cache: one workgroup
#pragma unroll
        for (int hh = 0; hh < HPW; ++hh)
#pragma unroll
            for (int b = 0; b < BMAX; ++b) {
                if (!(hh < nh && b < d.B) || j != d.k || c >= (d.Dh >> 3)) continue;
                const long at = (((long)b * d.H + h0 + hh) * d.steps + d.k) * d.Dh + 8 * c;
                *reinterpret_cast<u32x4*>(d.kc + at) = in[hh][b].k;
                *reinterpret_cast<u32x4*>(d.vc + at) = in[hh][b].v;
            }
    }
#pragma unroll
    for (int hh = 0; hh < HPW; ++hh)
#pragma unroll
        for (int b = 0; b < BMAX; ++b) {
            const bool on = hh < nh && b < d.B;                      // wave-uniform
            const u32x4 ov = mmi_dep_attn8_reduce(d, in[hh][b], lane);
            const int kl = (h0 + hh) * d.Dh + 8 * c - ks0 * 32;      // feature offset inside the wave's slice
            if (on && j == 0 && c < (d.Dh >> 3)) xs[wave][kl >> 5][((kl & 31) >> 3) * 16 + b] = ov;
        }
    __syncthreads();
    acc_t acc;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
    for (int u = 0; u < KPWMAX; ++u) {
        const u32x4 xv = (u < nks && (lane & 15) < d.B) ? xs[wave][u][lane] : zero;
        if (u < nks) acc = mmi_mfma_bf16_16x16x32(wv[u], xv, acc);
    }
    float accv[1][1][R];
#pragma unroll
    for (int r = 0; r < R; ++r) accv[0][0][r] = acc[r];
    mmi_gemm_epilogue<TN, 1, 1, WAVES>(a, accv, wave, lane, nt0, pre, nullptr, g_lo, g_hi);
}

// ------------------------------------------------------------------------------------------------
// sampling (sampling.py:86-106): softmax(logits/temp) -> top-k -> argmax(p / Exp(1)); greedy when disabled
// ------------------------------------------------------------------------------------------------
// One entry per streaming session (mmi_row_sampling + the engine's own words), 48 bytes = three 16-byte loads that k_sample
// requests with its other control words.  active == 0: the row samples with the handle's settings and the handle's counter.
// Active rows: Philox key = seed, counter (the row's stream offset, site, entry) - nothing of the slot, the batch size or the
// handle's age enters the draws.  The text site of an active row first patches its logits (bf16 in, fp32 arithmetic, bf16 out):
//   repetition penalty: every distinct in-vocabulary token among the newest rep_context entries of the row's ring of committed
//                       text tokens: l >= 0 ? l / penalty : l * penalty (correctly rounded fp32 division)
//   pad bias (sampling rows only, after the penalty): l_pad + pad_mult * temp_text, fp32 product then fp32 sum (no fma) - the
//                       reference multiplies the pad probability by exp(pad_mult) after the temperature softmax.  The sum is
//                       rounded to bf16 like every logit, so the bias resolves to one bf16 ulp of the pad logit.
#define MMI_TEXT_HIST 64
struct __attribute__((aligned(16))) RowSamp {
    int active, use_sampling, top_k, top_k_text;
    float temp, temp_text, pad_mult, rep_penalty;
    unsigned long long seed;
    int rep_context;          // 0 = off, <= MMI_TEXT_HIST
    unsigned hist_n;          // text tokens appended to the row's ring since it was emptied (k_lm_commit); slot = hist_n % 64
};

struct SampleArgs {
    const uint16_t* logits;   // [B][ld] bf16
    int ld, V, k;
    float temp;
    int use_sampling;
    const float* noise;       // [B][noise_ld] Exp(1) draws indexed by rank, used when *use_noise != 0
    int noise_ld;
    const int* use_noise;
    const unsigned long long* rng;   // [0] seed, [1] step counter
    int site;                 // which of the 1 + dep_q sampling sites (RNG stream id)
    int* out;                 // out[b * out_stride]
    int out_stride;
    int B;
    const int* forced;        // teacher forcing (parity taps / depformer_replace_tokens): forced[b * forced_stride]
    int forced_stride;        // is written instead of the sampled token when *use_forced != 0 and the value is >= 0
    const int* use_forced;
    // optional: the sampled token opens the next depth-transformer micro-step (lm.py:465-470) - the workgroup also writes
    // x0[b] = nx_pre[b] + nx_emb[token] (token -1 -> zero row, lm_utils.py:102-124) as the packed activation operand
    const uint16_t* nx_pre;   // [B][nx_ld] bf16: depformer_in[k](transformer_out), computed for all k ahead of the loop
    int nx_ld;
    const uint16_t* nx_emb;   // [card + 1][nx_D]
    uint16_t* nx_out;         // Xp layout (mmi_xp_index), null = nothing to write
    int nx_D, nx_T, nx_ksteps;
    int nx_dup;               // classifier-free guidance: the unconditioned twin of session b is model row b + nx_dup and
                              // opens the micro-step with the same token (lm.py:823-826 `input_.repeat(2, 1, 1)`); 0 = none
    // per-session sampling (mmi_lm_set_row_sampling): the table is read at run time, so a change never touches the launch list
    const RowSamp* rows;      // [B], never null
    const long* offsets;      // [B] the sessions' stream offsets: the Philox step counter of an active row
    const int* thist;         // [B][MMI_TEXT_HIST] ring of committed text tokens; non-null at the text site only
    int text;                 // 1 = the text site (temp_text / top_k_text of the row's entry)
    int pad_id;               // existing_text_padding_id: the entry RowSamp::pad_mult lifts
    // TTS machine (mmi_lm_enable_tts_machine): tts.py:553-555 `text_logits[..., pad] += padding_bonus` at the text site, every row
    int bonus_id;             // TokenIds.pad
    float bonus;              // 0 = off: the sampler's bits are those of a handle without the machine
};

__device__ __forceinline__ void mmi_sample_next_input(const SampleArgs& a, int b0, int tok) {
    if (!a.nx_out) return;
    const int per = a.nx_D / 8;
    for (int gg = (int)threadIdx.x; gg < (a.nx_dup ? 2 : 1) * per; gg += (int)blockDim.x) {
        const int g = gg % per, b = b0 + (gg / per) * a.nx_dup;
        const int n0 = 8 * g;
        const u32x4 pv = *reinterpret_cast<const u32x4*>(a.nx_pre + (long)b * a.nx_ld + n0);
        u32x4 ev = {0u, 0u, 0u, 0u};
        if (tok != -1) ev = *reinterpret_cast<const u32x4*>(a.nx_emb + (long)(tok < 0 ? 0 : tok) * a.nx_D + n0);
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = mmi_bf16_to_f32((uint16_t)(pv[e] & 0xffffu)) + mmi_bf16_to_f32((uint16_t)(ev[e] & 0xffffu));
            const float hi = mmi_bf16_to_f32((uint16_t)(pv[e] >> 16)) + mmi_bf16_to_f32((uint16_t)(ev[e] >> 16));
            ov[e] = mmi_pack_bf16x2(lo, hi);
        }
        *reinterpret_cast<u32x4*>(a.nx_out + mmi_xp_index(a.nx_T, b, n0, a.nx_ksteps)) = ov;
    }
}

// the depth transformer's first input row rebuilt from tok[b] (a step hook changed the text token after the sampler ran)
__global__ void k_dep_next_input(SampleArgs a, const int* __restrict__ tok) {
    mmi_sample_next_input(a, (int)blockIdx.x, tok[(long)blockIdx.x * a.out_stride]);
}

// The depth transformer's first input row of a demuxed text stream (demux_second_text_stream): x0[b] = nx_pre[b] +
// bf16(nx_emb[first] + emb2[second]) with the pair of k_lm_embed_demux, launched after the text sampler (and after an on_text_hook
// that may have replaced the token with a muxed one).  One workgroup per session.
__device__ __forceinline__ void mmi_sample_next_input_demux(const SampleArgs& a, int b0, int t0, const uint16_t* __restrict__ emb2, int N) {
    const int t = t0 < 0 ? 0 : t0;
    int second = t / N - 1;
    if (second > N - 1) second = N - 1;
    const int first = t % N;
    const int per = a.nx_D / 8;
    for (int gg = (int)threadIdx.x; gg < (a.nx_dup ? 2 : 1) * per; gg += (int)blockDim.x) {
        const int g = gg % per, b = b0 + (gg / per) * a.nx_dup;
        const int n0 = 8 * g;
        const u32x4 pv = *reinterpret_cast<const u32x4*>(a.nx_pre + (long)b * a.nx_ld + n0);
        u32x4 e1 = {0u, 0u, 0u, 0u}, e2 = {0u, 0u, 0u, 0u};
        if (t0 != -1) {
            e1 = *reinterpret_cast<const u32x4*>(a.nx_emb + (long)first * a.nx_D + n0);
            if (second >= 0) e2 = *reinterpret_cast<const u32x4*>(emb2 + (long)second * a.nx_D + n0);
        }
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float elo = mmi_bf16_to_f32((uint16_t)(e1[e] & 0xffffu)), ehi = mmi_bf16_to_f32((uint16_t)(e1[e] >> 16));
            if (second >= 0) {
                elo = mmi_round_bf16(elo + mmi_bf16_to_f32((uint16_t)(e2[e] & 0xffffu)));
                ehi = mmi_round_bf16(ehi + mmi_bf16_to_f32((uint16_t)(e2[e] >> 16)));
            }
            const float lo = mmi_bf16_to_f32((uint16_t)(pv[e] & 0xffffu)) + elo;
            const float hi = mmi_bf16_to_f32((uint16_t)(pv[e] >> 16)) + ehi;
            ov[e] = mmi_pack_bf16x2(lo, hi);
        }
        *reinterpret_cast<u32x4*>(a.nx_out + mmi_xp_index(a.nx_T, b, n0, a.nx_ksteps)) = ov;
    }
}
__global__ void k_dep_next_input_demux(SampleArgs a, const int* __restrict__ tok, const uint16_t* __restrict__ emb2, int N) {
    mmi_sample_next_input_demux(a, (int)blockIdx.x, tok[(long)blockIdx.x * a.out_stride], emb2, N);
}

__device__ __forceinline__ int mmi_apply_forced(const SampleArgs& a, int b, int tok) {
    if (*a.use_forced) {
        int f = a.forced[(long)b * a.forced_stride];
        if (f >= 0) return f;
    }
    return tok;
}

__device__ __forceinline__ void mmi_philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0,
                                                 unsigned k1) {
    unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
// Philox4x32-10, all four output words: counter (step, a, b), key = seed
__device__ __forceinline__ void mmi_philox4(unsigned long long seed, unsigned long long step, unsigned a, unsigned b, unsigned (&out)[4]) {
    unsigned c0 = (unsigned)step, c1 = (unsigned)(step >> 32), c2 = a, c3 = b;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        mmi_philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// Philox4x32-10 -> one Exp(1) draw
__device__ __forceinline__ float mmi_exp_noise(unsigned long long seed, unsigned long long step, unsigned a, unsigned b) {
    unsigned c0 = (unsigned)step, c1 = (unsigned)(step >> 32), c2 = a, c3 = b;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        mmi_philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    // (0, 1): 24 bits + 0.5 is rounded to fp32 above 2^23 (to even) and all-ones would arrive at 1.0f - a draw of -log(u) = 0 - without
    // the clamp to the largest float under 1; every other word keeps the value it always had
    float u = fminf(((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
    return -logf(u);
}

// exclusive prefix sum of one int per thread over the block; returns the block total through *total
template <int NT>
__device__ __forceinline__ int mmi_block_excl_scan(int v, int* wsum /* [NT/64 + 1] shared */, int* total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int o = mmi_shfl(inc, lane - d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) {
        int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// One block per session; thread t owns the E consecutive vocabulary entries [t*E, t*E+E) (NT*E >= V; V and the row
// stride multiples of 8), held packed in registers when CACHE (small vocabularies: the 8 depformer heads) or re-read
// from L2 in every pass (the 32000-entry text head).  The logits are bf16, so the top-k threshold is a 16-bit radix
// select (two 256-bin passes) on the order-preserving key of the logit - softmax is monotone in the logit - with ties
// at the threshold resolved towards the lower index; the probabilities p = softmax(logits/temp) are NOT renormalised
// over the top-k set (sampling.py:59-63,95-105), and the token is argmax_i p_i / q_rank(i), q ~ Exp(1) indexed by the
// rank of i in the descending top-k order, exactly the reference's `multinomial` trick (sampling.py:32-46).
__device__ __forceinline__ unsigned mmi_bf16_key(uint16_t h) {       // order-preserving: larger logit <-> larger key
    return (h & 0x8000u) ? (unsigned)(uint16_t)~h : (unsigned)(h | 0x8000u);
}

// One of the thread's E cached logits (entry `off` of its NV vectors) replaced in place: every (vector, word) is compared against
// `off` with compile-time indices, so the cache stays in registers (no dynamic register indexing, no scratch).
//   mode 0: repetition penalty p: l >= 0 ? l / p : l * p      mode 1: l + p (the pad bias, p = pad_mult * temp_text)
template <int NV>
__device__ __forceinline__ void mmi_sample_patch(u32x4 (&cache)[NV], int off, int mode, float p) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if ((off >> 1) == v * 4 + w) {
                const unsigned word = cache[v][w];
                const float l = mmi_bf16_to_f32((uint16_t)((off & 1) ? (word >> 16) : (word & 0xffffu)));
                const float r = mode == 0 ? (l >= 0.f ? l / p : l * p) : l + p;
                const unsigned nb = (unsigned)mmi_f32_to_bf16(r);
                cache[v][w] = (off & 1) ? ((word & 0x0000ffffu) | (nb << 16)) : ((word & 0xffff0000u) | nb);
            }
}

// entry `off` of the thread's cached logits, read with the same compile-time-indexed compares
template <int NV>
__device__ __forceinline__ uint16_t mmi_sample_peek(const u32x4 (&cache)[NV], int off) {
    unsigned word = 0u;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if ((off >> 1) == v * 4 + w) word = cache[v][w];
    return (uint16_t)((off & 1) ? (word >> 16) : (word & 0xffffu));
}

// a scheduling fence of the device compiler (nothing moves across it): keeps the unrolled per-entry expf / division chains of the
// nucleus select from being interleaved, which would spill the 128 registers a 1024-thread workgroup has
#if defined(__HIP_DEVICE_COMPILE__)
#define MMI_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define MMI_OPAQUE_F32(x) asm volatile("" : "+v"(x))      // the value as it is, its origin hidden from the optimiser
#define MMI_OPAQUE_U32(x) asm volatile("" : "+v"(x))
#else
#define MMI_SCHED_FENCE() ((void)0)
#define MMI_OPAQUE_F32(x) ((void)0)
#define MMI_OPAQUE_U32(x) ((void)0)
#endif
#ifndef MMI_SAMPLE_STAMP
#define MMI_SAMPLE_STAMP(i)          // scripts/sample_microbench.hip defines it: device-clock stamps at the kernel's stages
#endif
// Nucleus (top-p) sampling, DESIGN.md 8.17.  The sessions' effective (top_p, top_p_text) lie behind the row table, at
// a.rows + a.B: SampleArgs keeps its size and layout.  Only the NUC instantiations (k_sample_nucleus) read them.
struct __attribute__((aligned(8))) RowTopP { float top_p, top_p_text; };

// the bf16 logit of an order-preserving key (the inverse of mmi_bf16_key)
__device__ __forceinline__ uint16_t mmi_bf16_unkey(unsigned key) {
    return (key & 0x8000u) ? (uint16_t)(key & 0x7fffu) : (uint16_t)~key;
}

// The sampler's body is lm_sample_body.h, included into both kernels: as a shared __forceinline__ function template it changed the
// schedule of k_sample<1024, 32, true> (profiles/top_p/README.md); as included text with NUC = false k_sample keeps its device code.
template <int NT, int E, bool CACHE>
__global__ __launch_bounds__(NT) void k_sample(SampleArgs a) {
    constexpr bool NUC = false;
#include "lm_sample_body.h"
}
// the samplers of a handle with mmi_lm_enable_nucleus: rows whose top_p is 0 take the paths of k_sample
template <int NT, int E>
__global__ __launch_bounds__(NT) void k_sample_nucleus(SampleArgs a) {
    constexpr bool CACHE = true, NUC = true;
#include "lm_sample_body.h"
}

// mmi_lm_set_row_top_p / mmi_lm_clear_row_top_p: one session's entry of the table behind the row table
__global__ void k_lm_set_row_top_p(RowSamp* __restrict__ rows, int B, int session, float top_p, float top_p_text) {
    if (threadIdx.x == 0 && session >= 0 && session < B) reinterpret_cast<RowTopP*>(rows + B)[session] = RowTopP{top_p, top_p_text};
}

// ------------------------------------------------------------------------------------------------
// The TTS script machine on the device (mmi_lm_enable_tts_machine): models/tts.py:160-252 `StateMachine.process` and the three
// hooks of `TTSModel.generate` (tts.py:553-583), per session, read and written at run time like RowSamp and the row conditions.
// ------------------------------------------------------------------------------------------------
struct TtsParams {            // mmi_tts_params
    int text_card, new_word, pad, zero, second_stream_ahead, max_padding, initial_padding, delay_steps;
    float padding_bonus;
};
// One row of `stride` ints per session in the streaming-state arena: MMI_TTS_HDR header words, then
//   tokens[max_tokens] | entry_first[max_entries + 1] | entry_padding[max_entries] | consumption_times[max_entries] |
//   lookahead[max_tokens] | text_prefix[max_prefix] | audio_prefix[dep_q][max_prefix]
// `queued` is a slice (QPOS, QEND) of tokens[]: it is always a suffix of ONE entry's tokens, because a word is only taken when it
// is empty.  `lookahead_queued` can hold several words, so it is a real FIFO: a linear buffer with head / tail.  Every entry's
// tokens are appended to it at most once (word j appends the second_stream_ahead-th non-empty entry behind it, and that map is
// strictly increasing in j), so max_tokens slots cannot overflow and the indices never wrap.
enum {
    MMI_TTS_HAS = 0,          // 1 = the session has a script (else its sampled token passes through)
    MMI_TTS_NENT, MMI_TTS_TPLEN, MMI_TTS_APLEN,       // entries, text prefix columns, audio prefix columns
    MMI_TTS_NEXT,             // the next entry (State.entries as an index)
    MMI_TTS_REMAIN, MMI_TTS_FORCED,                   // remaining_padding, forced_padding
    MMI_TTS_QPOS, MMI_TTS_QEND, MMI_TTS_LAH, MMI_TTS_LAT,
    MMI_TTS_END,              // end_step, -1 = none
    MMI_TTS_NCONS,            // len(consumption_times)
    MMI_TTS_HDR = 16
};
struct TtsArgs {
    int* st;                  // [G][stride]
    int stride, max_entries, max_tokens, max_prefix;
    TtsParams p;
    const long* offsets;      // the session's own step counter (tts.py:602 `offset` when every row is in step)
    const uint8_t* exec;
    int* text_tok;            // [G] in: the sampled (or forced) token, out: the machine's
    const uint16_t* emb2;     // demuxed text stream: the second table of the depformer's text embedding, else null
    int demux_n;              // text_card + 1 of the demuxed stream
};
__device__ __forceinline__ int mmi_tts_off_first(int me, int mt) { return MMI_TTS_HDR + mt; }
__device__ __forceinline__ int mmi_tts_off_padding(int me, int mt) { return MMI_TTS_HDR + mt + me + 1; }
__device__ __forceinline__ int mmi_tts_off_times(int me, int mt) { return MMI_TTS_HDR + mt + 2 * me + 1; }
__device__ __forceinline__ int mmi_tts_off_look(int me, int mt) { return MMI_TTS_HDR + mt + 3 * me + 1; }
__device__ __forceinline__ int mmi_tts_off_tprefix(int me, int mt) { return MMI_TTS_HDR + 2 * mt + 3 * me + 1; }
__device__ __forceinline__ int mmi_tts_off_aprefix(int me, int mt, int mp) { return MMI_TTS_HDR + 2 * mt + 3 * me + 1 + mp; }

// new_state (tts.py:151-158) of the script the row holds
__device__ __forceinline__ void mmi_tts_rewind(int* r, int initial_padding) {
    r[MMI_TTS_NEXT] = 0; r[MMI_TTS_REMAIN] = initial_padding; r[MMI_TTS_FORCED] = initial_padding;
    r[MMI_TTS_QPOS] = 0; r[MMI_TTS_QEND] = 0; r[MMI_TTS_LAH] = 0; r[MMI_TTS_LAT] = 0;
    r[MMI_TTS_END] = -1; r[MMI_TTS_NCONS] = 0;
}

// StateMachine.process (tts.py:160-252) at step `step` on the sampled `token`; the text prefix first (tts.py:577-578).  One lane.
__device__ inline int mmi_tts_process(const TtsArgs& m, int* r, int step, int token) {
    const TtsParams& p = m.p;
    const int me = m.max_entries, mt = m.max_tokens;
    if (step < r[MMI_TTS_TPLEN]) return r[mmi_tts_off_tprefix(me, mt) + step];
    const int* toks = r + MMI_TTS_HDR;
    const int* first = r + mmi_tts_off_first(me, mt);
    const int* padding = r + mmi_tts_off_padding(me, mt);
    int* times = r + mmi_tts_off_times(me, mt);
    int* look = r + mmi_tts_off_look(me, mt);
    const int nent = r[MMI_TTS_NENT];
    int next = r[MMI_TTS_NEXT], remain = r[MMI_TTS_REMAIN], forced = r[MMI_TTS_FORCED];
    int qpos = r[MMI_TTS_QPOS], qend = r[MMI_TTS_QEND], lah = r[MMI_TTS_LAH], lat = r[MMI_TTS_LAT], end = r[MMI_TTS_END];
    if (token != p.new_word && token != p.pad) token = p.pad;                 // :174-175
    if (qpos < qend) token = p.pad;                                           // :177-185
    else if (forced > 0) token = p.pad;
    else if (remain <= 0) token = p.new_word;
    if (token == p.new_word) {                                                // :187-211
        if (next < nent) {
            const int e = next++;
            times[r[MMI_TTS_NCONS]] = step;
            r[MMI_TTS_NCONS] += 1;
            if (first[e + 1] > first[e]) {
                qpos = first[e]; qend = first[e + 1];
                if (p.second_stream_ahead) {                                  // get_tokens_ahead over what is left (:105-112)
                    int ahead = p.second_stream_ahead;
                    for (int j = next; j < nent; ++j)
                        if (first[j + 1] > first[j] && --ahead == 0) {
                            for (int t = first[j]; t < first[j + 1] && lat < mt; ++t) look[lat++] = toks[t];
                            break;
                        }
                }
                remain = p.max_padding;
            } else token = p.pad;                                             // a break: pretend the token was a pad
            forced = padding[e];
        } else {
            token = p.pad;
            if (p.second_stream_ahead && end < 0) token = p.new_word;
            if (end < 0) end = step;
        }
    }
    int out;
    if (token == p.pad) {                                                     // :214-224
        if (remain > 0) --remain;
        if (forced > 0) --forced;
        out = qpos < qend ? toks[qpos++] : p.pad;
    } else out = p.new_word;        // :225-230; the `zero` branch cannot be reached: :174-175 left only new_word and pad
    if (p.second_stream_ahead) {                                              // :232-249
        int second = -1;
        if (out == p.new_word) {
            second = p.new_word;
            out = qpos < qend ? toks[qpos++] : p.pad;
        } else if (lah < lat) second = look[lah++];
        out = (second + 1) * p.text_card + out;
    }
    r[MMI_TTS_NEXT] = next; r[MMI_TTS_REMAIN] = remain; r[MMI_TTS_FORCED] = forced;
    r[MMI_TTS_QPOS] = qpos; r[MMI_TTS_QEND] = qend; r[MMI_TTS_LAH] = lah; r[MMI_TTS_LAT] = lat; r[MMI_TTS_END] = end;
    return out;
}

// Behind the text sampler, one workgroup per session like k_dep_next_input: lane 0 runs the machine on text_tok[b] (a row whose
// exec mask is 0, or without a script, keeps its token and its state), then the whole workgroup writes the depth transformer's
// first input row from the machine's token - for the twin row under guidance too - which is what k_dep_next_input /
// k_dep_next_input_demux do: the machine rides in that launch instead of standing in front of it.  a.nx_out null: only the token
// (a model whose depformer_in runs per micro-step gathers the row in its GEMM).
__global__ __launch_bounds__(128) void k_tts_machine(SampleArgs a, TtsArgs m) {
    const int b = (int)blockIdx.x;
    MMI_SHARED int s_tok;
    if (threadIdx.x == 0) {
        int* r = m.st + (long)b * m.stride;
        int tok = m.text_tok[b];
        if (r[MMI_TTS_HAS] && m.exec[b]) {
            tok = mmi_tts_process(m, r, (int)m.offsets[b], tok);
            m.text_tok[b] = tok;
        }
        s_tok = tok;
    }
    __syncthreads();
    if (!a.nx_out) return;
    if (m.emb2) mmi_sample_next_input_demux(a, b, s_tok, m.emb2, m.demux_n);
    else mmi_sample_next_input(a, b, s_tok);
}

// ------------------------------------------------------------------------------------------------
// LMGen delay ring (lm.py:668-783)
// ------------------------------------------------------------------------------------------------
struct TokArgs {
    int* cache;            // [B][NC][CT]
    long* offsets;         // [B]
    const uint8_t* exec;   // [B]
    const int* delays;     // [NC]
    int B, NC, CT, dep_q, max_delay, card, text_card;
    RowSamp* rows;         // [B] per-session sampling table (mmi_lm_set_row_sampling)
    int* thist;            // [B][MMI_TEXT_HIST] ring of committed text tokens of the active rows
    int text_pad, text_eop;   // with text_card (the start token): the ids the ring skips (lm_generate_multistream.rs:151-157)
    // TTS machine (null = off): k_lm_reset rewinds a row, k_lm_commit applies the audio rule (tts_audio != 0)
    int* tts;                 // [B][tts_stride]
    int tts_stride, tts_aprefix, tts_max_prefix;      // tts_aprefix: where a row's audio prefix [dep_q][tts_max_prefix] starts
    int tts_zero, tts_delay_steps, tts_initial_padding, tts_audio;
};

// _on_audio_hook (tts.py:557-570) for codebook q of session b at step `off`: `zero` while the codebook's delay (+ delay_steps) has
// not passed, then the audio prefix column where it is not `ungenerated` - delayed per codebook as `_delayed` builds it
// (tts.py:115-121, 548-551: column off of codebook q holds prefix[q][off - delay]).
__device__ __forceinline__ int mmi_tts_audio_token(const TokArgs& t, int b, int q, long off, int tok) {
    const long dl = (long)t.delays[1 + q] + t.tts_delay_steps;
    if (off < dl) return t.tts_zero;
    const int* r = t.tts + (long)b * t.tts_stride;
    if (r[MMI_TTS_HAS] && off - dl < (long)r[MMI_TTS_APLEN]) {
        const int v = r[t.tts_aprefix + q * t.tts_max_prefix + (int)(off - dl)];
        if (v != -2) return v;
    }
    return tok;
}

// the audio rule in place on audio_tok, for a step that calls an on_audio_hook next to the machine (the hook sees the machine's
// tokens; the commit behind it then stores what the hook left)
__global__ void k_tts_audio_rule(TokArgs t, int* __restrict__ audio_tok) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= t.B * t.dep_q) return;
    const int b = idx / t.dep_q, q = idx % t.dep_q;
    if (t.exec[b]) audio_tok[idx] = mmi_tts_audio_token(t, b, q, t.offsets[b], audio_tok[idx]);
}

// 1. write the user's codes at (offset+delay)%CT, 2. gather the model input at offset%CT with init-token substitution
// 3. (threads past B*NC) the RoPE table of the step: (cos, sin)(offset[b] * max_period^(-2j/Dh)) for the new position of
//    every session (rope.py:11-82), computed once here instead of in each of the temporal layers' in_proj epilogues
__global__ void k_lm_prepare(TokArgs t, const int* __restrict__ user, int n_user, int* __restrict__ tokens, float* __restrict__ rope,
                             int Dh, float max_period) {
    int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= t.B * t.NC) {
        const int r = idx - t.B * t.NC;
        if (r < t.B * (Dh / 2)) {
            const int b = r / (Dh / 2), j = r - b * (Dh / 2);
            const float freq = expf((float)j * (-logf(max_period) * 2.0f / (float)Dh));
            const float ang = freq * (float)t.offsets[b];
            rope[2 * r] = cosf(ang);
            rope[2 * r + 1] = sinf(ang);
        }
        return;
    }
    const int b = idx / t.NC, c = idx % t.NC;
    const long off = t.offsets[b];
    const bool ex = t.exec[b] != 0;
    int* row = t.cache + ((long)b * t.NC + c) * t.CT;
    const int first_user = t.dep_q + 1;
    if (c >= first_user && ex) row[(int)((off + t.delays[c]) % t.CT)] = user[(long)b * n_user + (c - first_user)];
    const bool is_init = off <= (long)t.delays[c] || !ex;
    int tok = row[(int)(off % t.CT)];
    if (is_init) tok = c == 0 ? t.text_card : t.card;
    tokens[idx] = tok;
}

// The ring slots of a row whose offset, the step's included, is off_new: where the step's tokens are stored, and (declaring `i`)
// where site c of the returned frame is gathered.  k_step_logprob / k_lp_read (lm_logprob_kernels.h) keep their float rings by
// the same two.  The gather is a macro: as an inline function it moved two instructions of k_lm_commit's code.
__device__ __forceinline__ int mmi_ring_store_slot(long off_new, int CT) { return (int)(off_new % CT); }
#define MMI_RING_FRAME_SLOT(i, t, off_new, c)                   \
    long i = ((off_new) - (t).max_delay + (t).delays[c]) % (t).CT; \
    if (i < 0) i += (t).CT

// 4./5. advance offsets, store the sampled tokens, gather the delayed output frame
__global__ void k_lm_commit(TokArgs t, const int* __restrict__ text_tok, const int* __restrict__ audio_tok,
                            int* __restrict__ out, unsigned long long* __restrict__ rng) {
    int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b == 0) rng[1] += 1ull;
    if (b >= t.B) return;
    const bool ex = t.exec[b] != 0;
    const long off_new = t.offsets[b] + (ex ? 1 : 0);
    t.offsets[b] = off_new;
    const int pos = mmi_ring_store_slot(off_new, t.CT);
    int* rows = t.cache + (long)b * t.NC * t.CT;
    if (ex) {
        const int tt = text_tok[b];
        rows[pos] = tt;
        // TTS machine: the audio rule on the way into the ring (the depformer's own chain has used the sampled tokens, as in the
        // reference, where the hook runs after the depformer) - a variant of this kernel, not a launch of its own: a dependent
        // launch costs ~4.7 us whatever it computes, and the ring write is the only reader of the ruled tokens
        if (t.tts && t.tts_audio)
            for (int k = 0; k < t.dep_q; ++k) rows[(1 + k) * t.CT + pos] = mmi_tts_audio_token(t, b, k, off_new - 1, audio_tok[(long)b * t.dep_q + k]);
        else
        for (int k = 0; k < t.dep_q; ++k) rows[(1 + k) * t.CT + pos] = audio_tok[(long)b * t.dep_q + k];
        // the text history of an active row: the token the step stores (after forcing and after an on_text_hook)
        if (t.rows[b].active && tt != t.text_pad && tt != t.text_eop && tt != t.text_card) {
            const unsigned n = t.rows[b].hist_n;
            t.thist[(long)b * MMI_TEXT_HIST + (int)(n & (unsigned)(MMI_TEXT_HIST - 1))] = tt;
            t.rows[b].hist_n = n + 1u;
        }
    }
    const bool hide = off_new <= (long)t.max_delay || !ex;
    for (int c = 0; c <= t.dep_q; ++c) {
        MMI_RING_FRAME_SLOT(i, t, off_new, c);
        int v = rows[c * t.CT + (int)i];
        out[(long)b * (t.dep_q + 1) + c] = hide ? -2 : v;
    }
}

__global__ void k_i64_to_i32(const long* __restrict__ src, long src_rstride, int* __restrict__ dst, int rows, int cols) {
    int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= rows * cols) return;
    int r = idx / cols, c = idx % cols;
    dst[idx] = (int)src[(long)r * src_rstride + c];
}
__global__ void k_i32_to_i64(const int* __restrict__ src, long* __restrict__ dst, int n) {
    int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx < n) dst[idx] = (long)src[idx];
}
__global__ void k_bf16_to_f32(const uint16_t* __restrict__ src, float* __restrict__ dst, long n) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) dst[idx] = mmi_bf16_to_f32(src[idx]);
}
__global__ void k_fill_i32(int* __restrict__ p, int v, long n) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) p[idx] = v;
}
__global__ void k_lm_reset(TokArgs t, const uint8_t* __restrict__ mask, uint8_t* __restrict__ exec) {
    int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= t.B) return;
    if (mask && !mask[idx]) return;
    t.offsets[idx] = 0;           // lm.py:537-542; transformer.py:329-334 (KV end_offset, MHA offset)
    exec[idx] = 1;                // streaming.py:43-44
    t.rows[idx].hist_n = 0u;      // the row keeps its sampling settings; its text history starts over
    if (t.tts) mmi_tts_rewind(t.tts + (long)idx * t.tts_stride, t.tts_initial_padding);     // and its script, from new_state
}

// mmi_lm_set_row_sampling / mmi_lm_clear_row_sampling: up to 16 entries ride in the kernel arguments, so the call is
// stream-ordered without a host copy to wait for.  An entry with active == 0 returns the row to the handle's settings.
struct RowSampSet {
    RowSamp e[16];
    int row[16];
    int n;
};
__global__ void k_lm_set_rows(RowSamp* __restrict__ rows, RowSampSet set, int B) {
    const int i = (int)threadIdx.x;
    if (i >= set.n) return;
    const int r = set.row[i];
    if (r >= 0 && r < B) rows[r] = set.e[i];
}

// mmi_lm_set_row_condition: one session's cross-attention length, guidance coefficient and `sum` condition row(s); like
// k_lm_set_rows the scalars ride in the kernel arguments.  Under guidance (rows == 2) the session's twin G + b follows it.
// len / sum null: keep.  One workgroup per 256 features; the first thread of the first also writes the scalars.
struct RowCondSet {
    int session, G, rows;       // rows: model rows of a session (1, or 2 on a guided stream)
    int len;                    // 0 = keep
    float coef;
    const uint16_t* sum;        // [rows][D] or null = keep
    int D;
};
__global__ void k_lm_set_row_cond(int* __restrict__ len, float* __restrict__ coefs, uint16_t* __restrict__ cond, RowCondSet set) {
    const int d = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (d == 0) {
        coefs[set.session] = set.coef;
        if (len && set.len > 0)
            for (int r = 0; r < set.rows; ++r) len[r * set.G + set.session] = set.len;
    }
    if (cond && set.sum && d < set.D)
        for (int r = 0; r < set.rows; ++r) cond[(long)(r * set.G + set.session) * set.D + d] = set.sum[(long)r * set.D + d];
}

// ------------------------------------------------------------------------------------------------
// classifier-free guidance (lm.py:646-665, 712-733, 823-832) and extra heads (lm.py:793-807)
// ------------------------------------------------------------------------------------------------
// With cfg_coef != 1 the model runs 2G rows for G sessions: rows [0,G) conditioned, rows [G,2G) their unconditioned twins.
// After k_lm_prepare has built the G conditioned input rows, this kernel derives the twins: the same tokens, except
//   cfg_is_masked_until: every codebook reads the zero token (-1 -> zero embedding) while offset <= delay + masked_until[b],
//   cfg_is_no_text     : the text codebook reads the zero token,
// in both cases only where the row is past its initial token; it also replicates the per-session offset and RoPE angles
// onto the model rows (reset / exec masks reach the twins the same way: `.repeat(2)`, lm.py:655-663).
__global__ void k_lm_cfg_twins(TokArgs t, int* __restrict__ tokens, const int* __restrict__ masked_until, int no_text,
                               long* __restrict__ offsets_m, float* __restrict__ rope, int Dh) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int G = t.B;
    const int n_tok = G * t.NC, n_rope = G * Dh;
    if (idx < n_tok) {
        const int b = idx / t.NC, c = idx % t.NC;
        const long off = t.offsets[b];
        const bool is_init = off <= (long)t.delays[c] || !t.exec[b];
        int tok = tokens[idx];
        if (!is_init) {
            if (masked_until && off <= (long)t.delays[c] + (long)masked_until[b]) tok = -1;
            if (no_text && c == 0) tok = -1;
        }
        tokens[n_tok + idx] = tok;
    } else if (idx < n_tok + n_rope) {
        const int r = idx - n_tok;
        rope[n_rope + r] = rope[r];
    } else if (idx < n_tok + n_rope + G) {
        const int b = idx - n_tok - n_rope;
        offsets_m[b] = t.offsets[b];
        offsets_m[G + b] = t.offsets[b];
    }
}

// logits[b] <- logits_null + (logits - logits_null) * coef[b], each operation on bf16 tensors (lm.py:733, 830-832);
// logits rows [0,G) conditioned, [G,2G) unconditioned; the mix lands in row b, which the sampler and the taps then read.
// coefs [G]: one coefficient per session (mmi_lm_set_row_condition).  A session at coefficient 1 keeps its conditioned logits
// as they are - the reference does not mix there (lm.py:727), and n + bf16(bf16(l - n) * 1) is not l.
__global__ void k_cfg_mix(uint16_t* __restrict__ logits, int ld, int V, int G, const float* __restrict__ coefs) {
    const int b = blockIdx.y;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const float coef = coefs[b];
    if (i >= V || coef == 1.f) return;
    uint16_t* c = logits + (long)b * ld + i;
    const float l = mmi_bf16_to_f32(*c), n = mmi_bf16_to_f32(logits[(long)(G + b) * ld + i]);
    const float d = mmi_round_bf16(l - n);
    const float m = mmi_round_bf16(d * coef);
    *c = mmi_f32_to_bf16(n + m);
}

// softmax(extra_head(transformer_out)) (lm.py:803-806): one workgroup per (head, model row), one wave per output feature
// group; tout is the packed activation operand of the text head.  probs [rows][n_heads][hdim] fp32 (bf16 values).
__global__ __launch_bounds__(64) void k_extra_heads(const uint16_t* __restrict__ tout, int T, int ksteps, const uint16_t* __restrict__ w,
                                                   int D, int hdim, int n_heads, float* __restrict__ probs) {
    const int b = blockIdx.x, h = blockIdx.y, lane = (int)threadIdx.x;
    MMI_SHARED float lg[64];
    for (int j = 0; j < hdim; ++j) {
        const uint16_t* wr = w + ((long)h * hdim + j) * D;
        float acc = 0.f;
        for (int k = lane; k < D; k += 64) acc += mmi_bf16_to_f32(tout[mmi_xp_index(T, b, k, ksteps)]) * mmi_bf16_to_f32(wr[k]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += mmi_shfl_xor(acc, m);
        if (lane == 0) lg[j] = mmi_round_bf16(acc);          // nn.Linear output in bf16
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int j = 0; j < hdim; ++j) mx = fmaxf(mx, lg[j]);
    float den = 0.f;
    for (int j = 0; j < hdim; ++j) den += expf(lg[j] - mx);
    if (lane < hdim) probs[((long)b * n_heads + h) * hdim + lane] = mmi_round_bf16(expf(lg[lane] - mx) / den);
}
