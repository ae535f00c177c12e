// Log-probabilities of the stored tokens and top-N alternatives in the live step (mmi_lm_enable_logprobs).
//
// k_step_logprob is one launch in front of k_lm_commit: one workgroup per (session, site) reads the site's bf16 logits row as it
// stands when the op runs - after k_cfg_mix and after the sampler's written-back padding bonus, which is what the parity taps of
// the step return - and writes  ln softmax(row)[token]  of the token the step stores, plus the top_n entries first in the order
// (logit descending, index ascending), into float rings shaped like the delay ring, at the slot k_lm_commit is about to write the
// same step's tokens into.  Temperature, penalties, top-k and top-p play no part, as in mmi_lm_score.
//
// The token of site 0 is text_tok[b], of site k >= 1 audio_tok[b * dep_q + k - 1]: what mmi_lm_last_tokens returns after the step
// (after forcing and after the hooks).  Under the TTS machine that is the SAMPLED audio token even where the audio rule stores
// another one (the rule's tokens - `zero`, the audio prefix - are not the model's choice; they have no log-probability).
#pragma once
#include "lm_score_kernels.h"

#define MMI_LP_MAX_TOP 8
#define MMI_LP_NONE 0x7fffffff

struct LpRings {
    float* lp;                // [B][sites][CT]
    int* top_id;              // [B][sites][CT][top_n], null with top_n == 0
    float* top_lp;            // [B][sites][CT][top_n]
    int sites, top_n;
};

struct LpArgs {
    TokArgs t;                // the ring arithmetic of k_lm_commit: offsets, exec, CT.  The tap: offsets = exec = null, CT = 1 (slot 0)
    const uint16_t* text_logits;   // site 0: row b at text_logits + b * text_N
    int text_N;
    const uint16_t* dlogits;       // site k >= 1: row b at dlogits + (k - 1) * dstride + b * card
    long dstride;
    int card;
    const int* text_tok;      // [B]
    const int* audio_tok;     // [B][sites - 1]
    LpRings r;
};

// the fixed tree of k_score_logprob's maximum over (value, index) candidates: six butterfly steps in the wave, the four waves
// through LDS in wave order; the larger value wins, the lower index on a tie (an empty candidate is (-inf, MMI_LP_NONE))
__device__ __forceinline__ void mmi_lp_first(float& x, int& i, float* s_x, int* s_i, int lane, int wave) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float ox = mmi_shfl_xor(x, m);
        const int oi = mmi_shfl_xor(i, m);
        if (ox > x || (ox == x && oi < i)) { x = ox; i = oi; }
    }
    if (lane == 0) { s_x[wave] = x; s_i[wave] = i; }
    __syncthreads();
    x = s_x[0]; i = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_x[w] > x || (s_x[w] == x && s_i[w] < i)) { x = s_x[w]; i = s_i[w]; }
}

// ------------------------------------------------------------------------------------------------
// The register layout and the arithmetic of k_score_logprob (lm_score_kernels.h), term for term - thread t owns the 16-byte pieces
// t, t + 256, ... of the row, each loaded once; the maximum; the thread's own expf(x - max) in ascending index order, the six
// butterfly steps, (s0 + s1) + (s2 + s3); logp = (x_t - max) - logf(sum) - so that logp, and top_logp of any id, are the bits
// k_score_logprob gives for that row and target (the build has no fast-math and no contraction).
//
// The alternatives: every thread keeps ONE candidate, the first of its own entries in the order that is not selected yet (after
// the maximum pass: its own maximum).  A round is the tree over the 256 candidates; the thread that owned the winner rescans its
// pieces for its first entry behind the winner.  Comparisons are on the bf16 values widened exactly; no atomics, a fixed order.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MMI_SCORE_THREADS) void k_step_logprob(LpArgs a) {
    const int b = (int)blockIdx.x, s = (int)blockIdx.y, tid = (int)threadIdx.x;
    if (a.t.exec && !a.t.exec[b]) return;                 // the whole workgroup: a row that does not execute writes nothing
    const int lane = tid & 63, wave = tid >> 6;
    const int N = s == 0 ? a.text_N : a.card;
    const uint16_t* row = s == 0 ? a.text_logits + (long)b * a.text_N : a.dlogits + (long)(s - 1) * a.dstride + (long)b * a.card;
    const int tgt = s == 0 ? a.text_tok[b] : a.audio_tok[(long)b * (a.r.sites - 1) + (s - 1)];
    const int pieces = N / 8;
    u32x4 v[MMI_SCORE_PIECES];
#pragma unroll
    for (int j = 0; j < MMI_SCORE_PIECES; ++j) {
        const int c = tid + j * MMI_SCORE_THREADS;
        v[j] = u32x4{0u, 0u, 0u, 0u};
        if (c < pieces) v[j] = *reinterpret_cast<const u32x4*>(row + 8 * c);
    }
    float mx = -INFINITY, xt = 0.f;
    int mi = MMI_LP_NONE;
#pragma unroll
    for (int j = 0; j < MMI_SCORE_PIECES; ++j) {
        const int c = tid + j * MMI_SCORE_THREADS;
        if (c < pieces) {
            float f[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f[2 * q] = __builtin_bit_cast(float, v[j][q] << 16);
                f[2 * q + 1] = __builtin_bit_cast(float, v[j][q] & 0xffff0000u);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (f[e] > mx) { mx = f[e]; mi = 8 * c + e; }
                if (8 * c + e == tgt) xt = f[e];
            }
        }
    }
    if (mi == MMI_LP_NONE && tid < pieces) mi = 8 * tid;      // every entry of the thread is -inf: its first one stands for them
    MMI_SHARED float s_cx[2][4];
    MMI_SHARED int s_ci[2][4];
    MMI_SHARED float s_sum[4];
    MMI_SHARED float s_xt;
    const bool has_t = tgt >= 0 && tgt < N;
    if (has_t && ((tgt >> 3) & (MMI_SCORE_THREADS - 1)) == tid) s_xt = xt;       // the thread that owns the token's piece
    float cx = mx;            // the thread's candidate
    int ci = mi;
    float wx = cx;            // the round's winner
    int wi = ci;
    mmi_lp_first(wx, wi, s_cx[0], s_ci[0], lane, wave);
    mx = wx;
    // ---- sum of expf(x - max): the thread's terms in ascending index order, then the tree
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < MMI_SCORE_PIECES; ++j) {
        const int c = tid + j * MMI_SCORE_THREADS;
        if (c < pieces) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sum += expf(__builtin_bit_cast(float, v[j][q] << 16) - mx);
                sum += expf(__builtin_bit_cast(float, v[j][q] & 0xffff0000u) - mx);
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum += mmi_shfl_xor(sum, m);
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    const int slot = a.t.offsets ? mmi_ring_store_slot(a.t.offsets[b] + 1, a.t.CT) : 0;
    const long o = ((long)b * a.r.sites + s) * a.t.CT + slot;
    float lse = 0.f;
    if (tid == 0) {
        const float tot = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        lse = logf(tot);
        a.r.lp[o] = has_t ? (s_xt - mx) - lse : -INFINITY;
    }
    // ---- the alternatives: round r selects entry r of the order
    for (int r = 0; r < a.r.top_n; ++r) {
        if (r > 0) {
            if (ci == wi && wi != MMI_LP_NONE) {            // this thread owned the last winner: its first entry behind it
                float bx = -INFINITY;
                int bi = MMI_LP_NONE;
#pragma unroll
                for (int j = 0; j < MMI_SCORE_PIECES; ++j) {
                    const int c = tid + j * MMI_SCORE_THREADS;
                    if (c < pieces) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const unsigned w = v[j][e >> 1];
                            const float f = __builtin_bit_cast(float, (e & 1) ? (w & 0xffff0000u) : (w << 16));
                            const bool behind = f < wx || (f == wx && 8 * c + e > wi);
                            if (behind && (bi == MMI_LP_NONE || f > bx)) { bx = f; bi = 8 * c + e; }
                        }
                    }
                }
                cx = bx; ci = bi;
            }
            wx = cx; wi = ci;
            mmi_lp_first(wx, wi, s_cx[r & 1], s_ci[r & 1], lane, wave);
        }
        if (tid == 0) {
            a.r.top_id[o * a.r.top_n + r] = wi == MMI_LP_NONE ? -1 : wi;
            a.r.top_lp[o * a.r.top_n + r] = wi == MMI_LP_NONE ? NAN : (wx - mx) - lse;
        }
    }
}

// The rings of the named rows back to "nothing recorded": NaN / id -1.  mask (device, null = every row) as mmi_lm_reset takes it;
// n >= 0: the rows sess[0 .. n) instead, riding in the kernel arguments like a prefill pass's sessions.
struct LpClear {
    LpRings r;
    int CT, n;
    const uint8_t* mask;
    uint8_t sess[128];
};
__global__ void k_lp_clear(LpClear c) {
    const int b = c.n >= 0 ? (int)c.sess[blockIdx.x] : (int)blockIdx.x;
    if (c.mask && !c.mask[b]) return;
    const long per = (long)c.r.sites * c.CT, base = (long)b * per;
    for (long i = (long)threadIdx.x; i < per; i += (long)blockDim.x) c.r.lp[base + i] = NAN;
    for (long i = (long)threadIdx.x; i < per * c.r.top_n; i += (long)blockDim.x) {
        c.r.top_id[base * c.r.top_n + i] = -1;
        c.r.top_lp[base * c.r.top_n + i] = NAN;
    }
}

// The two read-outs (mmi_lm_last_logprobs / mmi_lm_frame_logprobs), behind the step's commit:
//   frame == 0  step coordinates: the slot of the row's last executed step, offsets[b] % CT - what mmi_lm_last_tokens lines up with;
//   frame != 0  frame coordinates: site c at k_lm_commit's own gather slot, NaN / -1 exactly where the frame the step returned
//               (out_i32) holds -2.
__global__ void k_lp_read(TokArgs t, LpRings r, const int* __restrict__ out_i32, int frame, float* __restrict__ logp,
                          int* __restrict__ top_id, float* __restrict__ top_lp) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= t.B * r.sites) return;
    const int b = idx / r.sites, c = idx - b * r.sites;
    const long off = t.offsets[b];
    const bool hidden = frame && out_i32[idx] == -2;
    MMI_RING_FRAME_SLOT(i, t, off, c);
    const int slot = frame ? (int)i : mmi_ring_store_slot(off, t.CT);
    const long o = (long)idx * t.CT + slot;
    logp[idx] = hidden ? NAN : r.lp[o];
    if (!top_id) return;
    for (int n = 0; n < r.top_n; ++n) {
        top_id[(long)idx * r.top_n + n] = hidden ? -1 : r.top_id[o * r.top_n + n];
        top_lp[(long)idx * r.top_n + n] = hidden ? NAN : r.top_lp[o * r.top_n + n];
    }
}
