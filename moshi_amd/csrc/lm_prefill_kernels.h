// Chunked prefill of known frames into a live session (mmi_lm_prefill): the kernels of one pass.
//
// A pass takes F frames of each of n sessions as R = n * F model rows, row r = i * F + f (session-major: the rows of a session are
// consecutive and so are their positions), once through the temporal transformer - no heads, no depth transformer, no samplers.
// The linears are the step's own GEMMs at R rows; what is new is the bookkeeping around them (k_pf_prepare, k_pf_embed,
// k_pf_commit_state), RoPE + ring format as a launch of its own (k_pf_rope_kv), the causal attention of a block of query rows
// (k_lm_attn_prefill) and the copy of the block into the ring behind it (k_pf_commit_kv).
//
// Why the block is staged: with a full ring, position p0 + 1 of a pass lands in the slot of position p0 + 1 - cap, which the query at
// p0 still attends.  So RoPE + quantisation write the block in RING FORMAT to a staging area, the attention reads older positions
// from the ring and the block's own positions from staging, and the commit launch moves the rows into their slots afterwards.
#pragma once
#include "lm_kernels.h"

struct PfArgs {
    int n, F;              // sessions of the call, frames of this pass
    int T;                 // frames of the whole call: the stride of the caller's arrays
    int f0;                // first frame of this pass inside them
    uint8_t sess[128];     // session of block i (a pass has at most 128 rows, a stream at most 128 sessions)
};

// The model input of every row, per k_lm_prepare's rule applied functionally (frame o = offsets[b] + f of session b, codebook c):
// the initial token while o <= delays[c]; a generated stream reads the token stored by frame o - 1, a user stream the code given at
// frame o - delays[c] - from the call's arrays where that frame lies inside this pass, from the delay ring where it lies before
// it (the previous pass, or the steps before the call, left it there).  Also the per-row tables: session, position, and the
// (cos, sin) of the position's angles in k_lm_prepare's own expression.
__global__ void k_pf_prepare(TokArgs t, PfArgs p, const long* __restrict__ user, int n_user, const long* __restrict__ toks,
                             int* __restrict__ tokens, int* __restrict__ row_sess, long* __restrict__ row_pos,
                             float* __restrict__ rope, int Dh, float max_period) {
    const int R = p.n * p.F;
    int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= R * t.NC) {
        const int q = idx - R * t.NC;
        if (q < R * (Dh / 2)) {
            const int r = q / (Dh / 2), j = q - r * (Dh / 2);
            const long pos = t.offsets[p.sess[r / p.F]] + (r % p.F);
            const float freq = expf((float)j * (-logf(max_period) * 2.0f / (float)Dh));
            const float ang = freq * (float)pos;
            rope[2 * q] = cosf(ang);
            rope[2 * q + 1] = sinf(ang);
        }
        return;
    }
    const int r = idx / t.NC, c = idx % t.NC;
    const int i = r / p.F, f = r - i * p.F;
    const int b = p.sess[i];
    const long o = t.offsets[b] + f;
    const int* ring = t.cache + ((long)b * t.NC + c) * t.CT;
    const int first_user = t.dep_q + 1;
    int tok;
    if (o <= (long)t.delays[c]) tok = c == 0 ? t.text_card : t.card;
    else if (c < first_user) tok = f >= 1 ? (int)toks[((long)i * first_user + c) * p.T + p.f0 + f - 1] : ring[(int)(o % t.CT)];
    else {
        const int fo = f - t.delays[c];
        tok = fo >= 0 ? (int)user[((long)i * n_user + (c - first_user)) * p.T + p.f0 + fo] : ring[(int)(o % t.CT)];
    }
    tokens[idx] = tok;
    if (c == 0) { row_sess[r] = b; row_pos[r] = o; }
}

// k_lm_embed / k_lm_embed_demux per row of a pass: the same sums in the same order, the `sum` condition taken from the row's session
__global__ void k_pf_embed(const int* __restrict__ tokens, int n_codebooks, const uint16_t* __restrict__ emb, int card1,
                           const uint16_t* __restrict__ text_t1, const uint16_t* __restrict__ text_t2, int N,
                           uint16_t* __restrict__ x, int D, int T, int ksteps, const uint16_t* __restrict__ cond,
                           const int* __restrict__ row_sess) {
    const int r = blockIdx.y;
    const int d = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (d >= D) return;
    const int* tk = tokens + (long)r * n_codebooks;
    float acc = 0.f;
    for (int c = 1; c < n_codebooks; ++c) {
        int t = tk[c];
        float v = 0.f;
        if (t != -1) v = mmi_bf16_to_f32(emb[((long)(c - 1) * card1 + (t < 0 ? 0 : t)) * D + d]);
        acc = c == 1 ? v : mmi_round_bf16(acc + v);
    }
    const int t0 = tk[0];
    float tv = 0.f;
    if (t0 != -1) {
        const int t = t0 < 0 ? 0 : t0;
        if (text_t2) {
            int second = t / N - 1;
            if (second > N - 1) second = N - 1;
            tv = mmi_bf16_to_f32(text_t1[(long)(t % N) * D + d]);
            if (second >= 0) tv = mmi_round_bf16(tv + mmi_bf16_to_f32(text_t2[(long)second * D + d]));
        } else tv = mmi_bf16_to_f32(text_t1[(long)t * D + d]);
    }
    acc = n_codebooks > 1 ? mmi_round_bf16(acc + tv) : tv;
    if (cond) acc = acc + mmi_bf16_to_f32(cond[(long)row_sess[r] * D + d]);
    x[mmi_xp_index(T, r, d, ksteps)] = mmi_f32_to_bf16(acc);
}

// What the call leaves in the token state of its sessions, one thread per session: the delay ring as the last CT frames of stepping
// would have left it (a frame writes one slot per codebook and the slots cycle with period CT, so the last CT frames own every slot
// the pass touched), the text history of rows with sampling settings of their own (k_lm_commit's rule, frame by frame), the last
// frame's tokens, the offset.  No output frame, and the handle's draw counter stays where it is.
__global__ void k_pf_commit_state(TokArgs t, PfArgs p, const long* __restrict__ user, int n_user, const long* __restrict__ toks,
                                  int* __restrict__ text_tok, int* __restrict__ audio_tok) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= p.n) return;
    const int b = p.sess[i];
    const long off0 = t.offsets[b];
    const int first_user = t.dep_q + 1;
    const int fa = p.F > t.CT ? p.F - t.CT : 0;
    for (int c = 0; c < t.NC; ++c) {
        int* ring = t.cache + ((long)b * t.NC + c) * t.CT;
        for (int f = fa; f < p.F; ++f) {
            const long o = off0 + f;
            if (c < first_user) ring[(int)((o + 1) % t.CT)] = (int)toks[((long)i * first_user + c) * p.T + p.f0 + f];
            else ring[(int)((o + t.delays[c]) % t.CT)] = (int)user[((long)i * n_user + (c - first_user)) * p.T + p.f0 + f];
        }
    }
    if (t.rows[b].active) {
        unsigned n = t.rows[b].hist_n;
        for (int f = 0; f < p.F; ++f) {
            const int tt = (int)toks[((long)i * first_user) * p.T + p.f0 + f];
            if (tt != t.text_pad && tt != t.text_eop && tt != t.text_card) {
                t.thist[(long)b * MMI_TEXT_HIST + (int)(n & (unsigned)(MMI_TEXT_HIST - 1))] = tt;
                n += 1u;
            }
        }
        t.rows[b].hist_n = n;
    }
    const int fl = p.f0 + p.F - 1;
    text_tok[b] = (int)toks[((long)i * first_user) * p.T + fl];
    for (int k = 0; k < t.dep_q; ++k) audio_tok[(long)b * t.dep_q + k] = (int)toks[((long)i * first_user + 1 + k) * p.T + fl];
    t.offsets[b] = off0 + p.F;
}

// mmi_lm_last_tokens: the tokens the last step (or prefill) stored, [B][1 + dep_q] int64 in step coordinates
__global__ void k_pf_last_tokens(const int* __restrict__ text_tok, const int* __restrict__ audio_tok, int B, int dep_q, long* __restrict__ out) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= B * (1 + dep_q)) return;
    const int b = idx / (1 + dep_q), c = idx - b * (1 + dep_q);
    out[idx] = c == 0 ? (long)text_tok[b] : (long)audio_tok[(long)b * dep_q + c - 1];
}

// ------------------------------------------------------------------------------------------------
// RoPE + ring format of a pass: qkv [R][3 H Dh] (the in_proj output, bf16 - MMI_EPI_STORE rounds where MMI_EPI_ROPE_KV does) ->
// q [R][H][Dh] roped bf16, the attention's operand; k (roped) and v in the RING's format into the staged block
// [R][H][row bytes] (+ a 4-bit ring's scale bytes [R][H][Dh / 16]) - the bytes MMI_EPI_ROPE_KV would store: the same rotation
// (mmi_rope_rotate), the same conversions (mmi_cvt_fp8x4; mmi_kv4_absmax8 / _scale_byte / _quant8).  One thread per 16 features.
// ------------------------------------------------------------------------------------------------
struct PfRopeArgs {
    const uint16_t* qkv;
    const float* rope;     // [R][Dh / 2][2]
    uint16_t* q;
    uint8_t *sk, *sv;      // staged codes
    uint8_t *sks, *svs;    // staged scale bytes (4-bit ring)
    int R, H, Dh;
};

template <int KVF>
__global__ void k_pf_rope_kv(PfRopeArgs a) {
    const int HD = a.H * a.Dh, per_row = 3 * HD / 16;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)a.R * per_row) return;
    const int r = (int)(idx / per_row), n0 = (int)(idx - (long)r * per_row) * 16;
    const int sec = n0 / HD, hn = n0 - sec * HD, h = hn / a.Dh, d0 = hn - h * a.Dh;
    const uint16_t* src = a.qkv + (long)r * 3 * HD + n0;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(src), hi = *reinterpret_cast<const u32x4*>(src + 8);
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[2 * q] = mmi_bf16_to_f32((uint16_t)(lo[q] & 0xffffu));
        v[2 * q + 1] = mmi_bf16_to_f32((uint16_t)(lo[q] >> 16));
        v[8 + 2 * q] = mmi_bf16_to_f32((uint16_t)(hi[q] & 0xffffu));
        v[8 + 2 * q + 1] = mmi_bf16_to_f32((uint16_t)(hi[q] >> 16));
    }
    if (sec < 2) {
        const float* cs = a.rope + ((long)r * (a.Dh / 2) + d0 / 2) * 2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float re = v[2 * j], im = v[2 * j + 1];
            mmi_rope_rotate(re, im, cs[2 * j], cs[2 * j + 1], v[2 * j], v[2 * j + 1]);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = mmi_round_bf16(v[e]);
    if (sec == 0) {
        u32x4 o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o0[e] = mmi_pack_bf16x2(v[2 * e], v[2 * e + 1]); o1[e] = mmi_pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]); }
        uint16_t* dst = a.q + (long)r * HD + hn;
        *reinterpret_cast<u32x4*>(dst) = o0;
        *reinterpret_cast<u32x4*>(dst + 8) = o1;
        return;
    }
    const long row = (long)r * a.H + h;
    uint8_t* plane = sec == 1 ? a.sk : a.sv;
    if constexpr (KVF == 2) {
        const uint32_t am0 = mmi_kv4_absmax8(v), am1 = mmi_kv4_absmax8(v + 8);
        const uint32_t sb = mmi_kv4_scale_byte(am0 > am1 ? am0 : am1);
        u32x2 c = {0u, 0u};
        if (sb) { c[0] = mmi_kv4_quant8(v, sb); c[1] = mmi_kv4_quant8(v + 8, sb); }
        *reinterpret_cast<u32x2*>(plane + row * (a.Dh / 2) + d0 / 2) = c;
        (sec == 1 ? a.sks : a.svs)[row * (a.Dh / 16) + d0 / 16] = (uint8_t)sb;
    } else if constexpr (KVF == 1) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = mmi_cvt_fp8x4(v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]);
        *reinterpret_cast<u32x4*>(plane + row * a.Dh + d0) = o;
    } else {
        u32x4 o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o0[e] = mmi_pack_bf16x2(v[2 * e], v[2 * e + 1]); o1[e] = mmi_pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]); }
        uint8_t* dst = plane + (row * a.Dh + d0) * 2;
        *reinterpret_cast<u32x4*>(dst) = o0;
        *reinterpret_cast<u32x4*>(dst + 16) = o1;
    }
}

// ------------------------------------------------------------------------------------------------
// The attention of a pass.  Operands and geometry shared by the attention and the commit of the block.
// ------------------------------------------------------------------------------------------------
struct PfAttnArgs {
    const uint16_t* q;         // [R][H][Dh] roped queries
    uint8_t *kc, *vc;          // the layer's ring: [rings][H][cap][row bytes]
    long kv_soff;              // 4-bit ring: bytes from a codes plane to its scale plane [rings][H][cap][Dh / 16]
    const uint8_t *sk, *sv;    // staged block [R][H][row bytes]
    const uint8_t *sks, *svs;  // 4-bit: its scale bytes [R][H][Dh / 16]
    const int* row_sess;       // [R] ring of the row (constant over a session's block)
    const long* row_pos;       // [R] position of the row (consecutive over a session's block)
    uint16_t* out;             // packed (T, out_ksteps) activations of out_proj, feature = h * Dh + d
    int T, out_ksteps;
    int H, cap, context;
    int n, F;                  // R = n * F
};

#define MMI_PF_QT 32           // query rows of a tile = key rows of a tile (one 32x32 MFMA block)

// Causal attention of a block of query rows of one session over the ring's older positions and the staged block.
// grid (n * ceil(F / 32), H), 256 threads.  A workgroup owns 32 query rows of one (session, head); its 4 waves deal the key tiles
// (32 rows: first the ring's written slots 0 .. L - 1, L = min(p0, cap), then the staged rows up to the tile's last query) out
// round-robin, every wave with an online softmax of its own, merged once at the end through LDS in a fixed order.  A key / value
// row is loaded once per query tile - not once per query, which is what a decode kernel run per frame would do.
//   scores   S^T = K Q^T on the bf16 MFMA (v_mfma_f32_32x32x16_bf16; e4m3 and 4-bit keys widened exactly to bf16), fp32 sums: a
//            lane then holds 16 keys of ONE query (l & 31), lanes l and l ^ 32 the two halves of the tile - the softmax is in-lane
//            plus one cross-half exchange
//   P V      O^T = V^T P^T on the fp32 MFMA (v_mfma_f32_32x32x2f32): P stays fp32 (the decode kernels' error model), the P values
//            sit in the lanes the B operand wants them in, and the accumulator's column is the lane's query, so the rescale is
//            in-lane.  V^T comes from a wave-private LDS tile the wave widened to fp32 (32 x Dh floats: 64 KiB per workgroup at
//            Dh = 128, where the registers - 320 VGPRs - leave one workgroup per CU; profiles/prefill/README.md).  The waves share
//            nothing before the merge, yet the two barriers of the loop are block-wide (the device vocabulary has no wave-level
//            fence): hence the block-uniform trip count with dead tiles.
// Mask: the reference's rule as attn_cases.valid_mask states it - slot s holds position p0 - 1 + d (d = s - (p0 - 1) % cap <= 0) or
// p0 - 1 + d - cap, staged row j position p0 + j; query at p attends pos iff 0 <= p - pos < context.  Every load is unconditional
// from a clamped row (ring: L - 1, staged: the tile's last query row); a masked score is replaced by -inf, never computed with, and
// a value row that no query of the tile attends is stored to LDS as zeros - no result depends on a never-written slot or on a staged
// row behind the tile.  Causality is per query: in the diagonal tile, where a staged row lies behind some of the tile's queries, P V
// runs per (query, key) under the mask (see there), so a frame's K / V never reaches an earlier frame's output.  What is left is
// the window: a written row that the window of SOME queries of a tile has left is used as 0 * v by those, as in the decode kernels.
template <int DH, int KVF>
__global__ __launch_bounds__(256) void k_lm_attn_prefill(PfAttnArgs a) {
    constexpr int EPL = KVF == 2 ? 32 : (KVF == 1 ? 16 : 8);          // elements of a 16-byte chunk
    constexpr int ROWB = KVF == 2 ? DH / 2 : (KVF == 1 ? DH : 2 * DH);
    constexpr int CPR = ROWB / 16;                                     // chunks per row
    constexpr int NCH = (32 * CPR + 63) / 64;                          // value chunks per lane and tile
    constexpr int KC = DH / 16, DB = DH / 32;
    MMI_SHARED __attribute__((aligned(16))) float sV[4 * 32 * DH];     // per wave: the value tile [key][d]; at the end: O^T [d][query]
    MMI_SHARED float sm[4 * 32];
    MMI_SHARED float sl[4 * 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, qi = lane & 31, half = lane >> 5;
    const int tiles_per = (a.F + MMI_PF_QT - 1) / MMI_PF_QT;
    const int blk = (int)blockIdx.x / tiles_per, tq = (int)blockIdx.x - blk * tiles_per, h = blockIdx.y;
    const int blk0 = blk * a.F, q0 = tq * MMI_PF_QT;
    const int lastq = min(q0 + MMI_PF_QT, a.F) - 1;                    // the tile's last query row (inside the block)
    const int b = a.row_sess[blk0];
    const long p0 = a.row_pos[blk0];
    const int L = (int)(p0 < (long)a.cap ? p0 : (long)a.cap);
    const int end_prev = L > 0 ? (int)((p0 - 1) % a.cap) : 0;
    const long pq = p0 + min(q0 + qi, lastq), pq_min = p0 + q0;
    const int NRT = (L + 31) / 32, NT = NRT + tq + 1;
    // key row kk of tile g: where it is loaded from (clamped), its position, and whether it exists
    struct Row { long at; long pos; bool live; bool ring; };
    auto row_of = [&](int g, int kk) {
        Row r;
        if (g < NRT) {
            const int slot = 32 * g + kk, sc = min(slot, L - 1);
            const int delta = slot - end_prev;
            r.pos = delta <= 0 ? p0 - 1 + delta : p0 - 1 + delta - a.cap;
            r.live = slot < L && r.pos >= 0;
            r.at = ((long)b * a.H + h) * a.cap + sc;
            r.ring = true;
        } else {
            const int ts = min(g - NRT, tq), srow = 32 * ts + kk;
            r.pos = p0 + srow;
            r.live = g < NT && srow <= lastq;
            r.at = ((long)blk0 + min(srow, lastq)) * a.H + h;
            r.ring = false;
        }
        return r;
    };
    u32x4 qf[KC];
    {
        const uint16_t* qp = a.q + (((long)blk0 + min(q0 + qi, lastq)) * a.H + h) * DH + 8 * half;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) qf[kc] = *reinterpret_cast<const u32x4*>(qp + 16 * kc);
    }
    const float scale = 1.0f / sqrtf((float)DH);
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
    float* myV = sV + wave * 32 * DH;
    const int iters = (NT + 3) / 4;                                    // block-uniform: a wave past its last tile runs a dead one
    for (int it = 0; it < iters; ++it) {
        const int g = it * 4 + wave;
        // ---- keys: 8 elements of key row (lane & 31) per 16-wide k-chunk, as bf16
        const Row kr = row_of(g, qi);
        u32x4 kf[KC];
        {
            const uint8_t* kb = (kr.ring ? a.kc : a.sk) + kr.at * ROWB;
            if constexpr (KVF == 0) {
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) kf[kc] = *reinterpret_cast<const u32x4*>(kb + (16 * kc + 8 * half) * 2);
            } else if constexpr (KVF == 1) {
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    const u32x2 w = *reinterpret_cast<const u32x2*>(kb + 16 * kc + 8 * half);
                    float f[8];
                    mmi_fp8x4_to_f32(w[0], f);
                    mmi_fp8x4_to_f32(w[1], f + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) kf[kc][e] = mmi_pack_bf16x2(f[2 * e], f[2 * e + 1]);
                }
            } else {
                const uint8_t* ks = (kr.ring ? a.kc + a.kv_soff : a.sks) + kr.at * (DH / 16);
#pragma unroll
                for (int kc = 0; kc < KC; ++kc)
                    kf[kc] = mmi_fp4x8_to_bf16(*reinterpret_cast<const uint32_t*>(kb + 8 * kc + 4 * half), (uint32_t)ks[kc]);
            }
        }
        // ---- values: the tile's 32 rows in 16-byte chunks, widened to fp32
        u32x4 vv[NCH];
        uint32_t vs[NCH];
        bool vlive[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = min(lane + 64 * c, 32 * CPR - 1), kk = ch / CPR, seg = ch - kk * CPR;
            const Row vr = row_of(g, kk);
            vv[c] = *reinterpret_cast<const u32x4*>((vr.ring ? a.vc : a.sv) + vr.at * ROWB + seg * 16);
            if constexpr (KVF == 2)
                vs[c] = *reinterpret_cast<const uint16_t*>((vr.ring ? a.vc + a.kv_soff : a.svs) + vr.at * (DH / 16) + seg * 2);
            else vs[c] = 0u;
            vlive[c] = vr.live && pq_min - vr.pos < (long)a.context;       // some query of the tile may attend it
        }
        __syncthreads();                                               // the previous tile's P V has read the LDS tile
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + 64 * c;
            if (ch >= 32 * CPR) continue;
            const int kk = ch / CPR, seg = ch - kk * CPR;
            float f[EPL];
            if constexpr (KVF == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) mmi_kv4_widen8(vv[c][q], (vs[c] >> (8 * (q >> 1))) & 0xffu, f + 8 * q);
            } else if constexpr (KVF == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) mmi_fp8x4_to_f32(vv[c][q], f + 4 * q);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f[2 * q] = mmi_bf16_to_f32((uint16_t)(vv[c][q] & 0xffffu));
                    f[2 * q + 1] = mmi_bf16_to_f32((uint16_t)(vv[c][q] >> 16));
                }
            }
            float* dst = myV + kk * DH + seg * EPL;
#pragma unroll
            for (int e = 0; e < EPL; e += 4) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (vlive[c]) o = f32x4{f[e], f[e + 1], f[e + 2], f[e + 3]};
                *reinterpret_cast<f32x4*>(dst + e) = o;
            }
        }
        // ---- scores of the lane's query against its 16 keys of the tile
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) s = mmi_mfma_bf16_32x32x16(kf[kc], qf[kc], s);
        float mx = -INFINITY;
        uint32_t vbits = 0u;                                           // bit r: the lane's query attends its key r of the tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const Row sr = row_of(g, (r & 3) + 8 * (r >> 2) + 4 * half);
            const long dq = pq - sr.pos;
            const bool valid = sr.live && dq >= 0 && dq < (long)a.context;
            vbits |= valid ? 1u << r : 0u;
            s[r] = valid ? s[r] * scale : -INFINITY;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, mmi_shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float resc = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = (m_new == -INFINITY) ? 0.f : expf(s[r] - m_new);
            psum += s[r];
        }
        l_run = l_run * resc + psum;                                   // this half's share; the halves are added at the end
        m_run = m_new;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[db][r] *= resc;
        __syncthreads();                                               // the LDS tile is complete
        if (g == NT - 1) {
            // ---- the DIAGONAL tile (the staged rows of the tile's own queries): a row behind a query must not reach that query's
            // output even as 0 * v - stepping computes frame f before frame f + 1 exists - so here P V is an fp32 fma chain per
            // (query, key) under the score's own mask, on the VALU: 32 keys x Dh / 2 features per lane, once per workgroup.  The
            // other half-wave's P and mask come over by one exchange each; a key's value row is an LDS broadcast.
            const uint32_t obits = mmi_shfl_xor(vbits, 32);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float po = mmi_shfl_xor(s[r], 32);
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const bool mine = hh == half;
                    const float pv = mine ? s[r] : po;
                    if (!(((mine ? vbits : obits) >> r) & 1u)) continue;
                    const float* vrow = myV + ((r & 3) + 8 * (r >> 2) + 4 * hh) * DH + 4 * half;
#pragma unroll
                    for (int db = 0; db < DB; ++db)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const f32x4 v4 = *reinterpret_cast<const f32x4*>(vrow + 32 * db + 8 * c);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[db][4 * c + e] = mmi_fma(v4[e], pv, acc[db][4 * c + e]);
                        }
                }
            }
            continue;
        }
        // ---- O^T += V^T P^T: step r pairs the keys (r & 3) + 8 (r >> 2) and + 4, which lanes < 32 and >= 32 hold for query l & 31
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vrow = myV + ((r & 3) + 8 * (r >> 2) + 4 * half) * DH + qi;
#pragma unroll
            for (int db = 0; db < DB; ++db) acc[db] = mmi_mfma_f32_32x32x2(vrow[32 * db], s[r], acc[db]);
        }
    }
    // ---- merge the four waves (fixed order) and write the tile's rows
    __syncthreads();
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) myV[(32 * db + (r & 3) + 8 * (r >> 2) + 4 * half) * 32 + qi] = acc[db][r];
    sl[wave * 64 + lane] = l_run;
    if (half == 0) sm[wave * 32 + qi] = m_run;
    __syncthreads();
    {
        const int q = tid & 31, dg = tid >> 5;
        float mt = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mt = fmaxf(mt, sm[w * 32 + q]);
        float ws[4], lt = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = sm[w * 32 + q];
            ws[w] = mw == -INFINITY ? 0.f : expf(mw - mt);
            lt += ws[w] * (sl[w * 64 + q] + sl[w * 64 + 32 + q]);
        }
        if (q0 + q <= lastq) {
            for (int d = dg * (DH / 8); d < (dg + 1) * (DH / 8); ++d) {
                float o = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) o += ws[w] * sV[(w * DH + d) * 32 + q];
                a.out[mmi_xp_index(a.T, blk0 + q0 + q, h * DH + d, a.out_ksteps)] = mmi_f32_to_bf16(o / lt);
            }
        }
    }
}

// The staged block into the ring, behind the attention: row r of session b goes to slot row_pos[r] % cap of ring row_sess[r].  A
// pass of more than cap frames meets a slot more than once: only the last row that maps to it is copied.  One thread per 16 bytes.
template <int KVF>
__global__ void k_pf_commit_kv(PfAttnArgs a, int Dh) {
    const int ROWB = KVF == 2 ? Dh / 2 : (KVF == 1 ? Dh : 2 * Dh), CPR = ROWB / 16;
    const int R = a.n * a.F;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)R * a.H * CPR) return;
    const int seg = (int)(idx % CPR);
    const long rh = idx / CPR;
    const int r = (int)(rh / a.H), h = (int)(rh - (long)r * a.H);
    if (r % a.F + a.cap < a.F) return;
    const long dst = ((long)a.row_sess[r] * a.H + h) * a.cap + (int)(a.row_pos[r] % a.cap);
    *reinterpret_cast<u32x4*>(a.kc + dst * ROWB + seg * 16) = *reinterpret_cast<const u32x4*>(a.sk + rh * ROWB + seg * 16);
    *reinterpret_cast<u32x4*>(a.vc + dst * ROWB + seg * 16) = *reinterpret_cast<const u32x4*>(a.sv + rh * ROWB + seg * 16);
    if constexpr (KVF == 2) {
        if (seg == 0)
            for (int j = 0; j < Dh / 16; ++j) {
                a.kc[a.kv_soff + dst * (Dh / 16) + j] = a.sks[rh * (Dh / 16) + j];
                a.vc[a.kv_soff + dst * (Dh / 16) + j] = a.svs[rh * (Dh / 16) + j];
            }
    }
}
