// Teacher-forced scoring of known frames on the prefill path (mmi_lm_score): the kernels a scoring pass adds to
// the pass of lm_prefill_kernels.h.
//
// A scoring pass runs the prefill pass to its end (the last layer's attention, out_proj, FFN and out_norm), then the text head and
// the depth transformer on the same R = n * F rows, as dep_q micro-steps in sequence.  Under forcing micro-step k's input token is
// GIVEN (site k - 1 of the same frame), so the rows never wait for a sampler: k_sc_targets gathers the given tokens of the pass
// into a table, k_sc_dep_input builds a micro-step's input rows from it, and k_score_logprob turns a row of bf16 logits into the
// log-probability of its given token, the argmax and (optionally) the row widened to fp32.  Nothing is sampled.
#pragma once
#include "lm_prefill_kernels.h"

// The given tokens of the pass as a table [R][1 + dep_q] (site 0 = text): row r = i * F + f reads frame f0 + f of block i
__global__ void k_sc_targets(PfArgs p, int sites, const long* __restrict__ toks, int* __restrict__ targets) {
    const int R = p.n * p.F;
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= R * sites) return;
    const int r = idx / sites, c = idx - r * sites;
    const int i = r / p.F, f = r - i * p.F;
    targets[idx] = (int)toks[((long)i * sites + c) * p.T + p.f0 + f];
}

// Micro-step k's packed input row of every row of the pass: x0[r] = pre[r] + emb[token] with the token GIVEN - the frame's text
// token (k = 0, site 0) or audio token k - 1 (site k) - where the step takes its sampler's output (mmi_sample_next_input: the same
// sums at the same rounding points; token -1 -> zero row, lm_utils.py:102-124).  One workgroup per row, one thread per 8 features.
struct ScDepInArgs {
    const uint16_t* pre;      // [R][ld] bf16: depformer_in[sched[k]](transformer_out)
    int ld;
    const uint16_t* emb;      // [card + 1][D] (k = 0: the text table)
    const int* targets;       // [R][sites]
    int sites, site;
    uint16_t* out;            // packed (T, ksteps)
    int D, T, ksteps;
};
__global__ void k_sc_dep_input(ScDepInArgs a) {
    const int r = (int)blockIdx.x;
    const int tok = a.targets[(long)r * a.sites + a.site];
    for (int g = (int)threadIdx.x; g < a.D / 8; g += (int)blockDim.x) {
        const int n0 = 8 * g;
        const u32x4 pv = *reinterpret_cast<const u32x4*>(a.pre + (long)r * a.ld + n0);
        u32x4 ev = {0u, 0u, 0u, 0u};
        if (tok != -1) ev = *reinterpret_cast<const u32x4*>(a.emb + (long)(tok < 0 ? 0 : tok) * a.D + n0);
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = mmi_bf16_to_f32((uint16_t)(pv[e] & 0xffffu)) + mmi_bf16_to_f32((uint16_t)(ev[e] & 0xffffu));
            const float hi = mmi_bf16_to_f32((uint16_t)(pv[e] >> 16)) + mmi_bf16_to_f32((uint16_t)(ev[e] >> 16));
            ov[e] = mmi_pack_bf16x2(lo, hi);
        }
        *reinterpret_cast<u32x4*>(a.out + mmi_xp_index(a.T, r, n0, a.ksteps)) = ov;
    }
}

// ------------------------------------------------------------------------------------------------
// log softmax(logits)[given token], argmax and the fp32 copy of one bf16 logits row of N <= 32768 entries (N % 8 == 0).
// One workgroup of 256 threads per (row, site).  Thread t owns the 16-byte pieces t, t + 256, ... of the row - at most 16 of
// them, loaded once and kept in registers - so its values are in ascending index order:
//   max     per thread, then a fixed tree (6 butterfly steps in the wave, the four waves through LDS);
//   argmax  the lowest index among the largest: a thread keeps the first of its own, the tree prefers the lower index on a tie;
//   sum     of expf(x - max) in fp32: the thread's own terms in ascending index order (at most N / 256), then the same fixed tree.
//           No atomics: the same bytes on every run;
//   logp    (x_t - max) - logf(sum); a token outside [0, N) gives -inf.  A NaN logit: fmaxf drops it from the maximum, expf
//           carries it into the sum, so logp is NaN (argmax is then unspecified).
// ------------------------------------------------------------------------------------------------
#define MMI_SCORE_THREADS 256
#define MMI_SCORE_PIECES 16        // 16-byte pieces per thread: N <= 8 * 256 * 16
struct ScoreArgs {
    const uint16_t* logits;   // site s, row r at logits + s * site_stride + r * ld
    long site_stride;
    int ld, N;
    const int* targets;       // the given token of (r, s) at targets[r * tgt_stride + tgt_off + s]
    int tgt_stride, tgt_off;
    float* logp;              // outputs of (r, s) at [orow(r) * out_stride + out_off + s]
    int* argmax;              // null = not wanted
    int out_stride, out_off;
    float* lf32;              // null, or the row widened to fp32 at lf32 + orow(r) * lf32_row + s * lf32_site
    long lf32_row, lf32_site;
    int F, Tall, f0;          // orow(r) = (r / F) * Tall + f0 + r % F: the pass's rows inside the call's [n][T] arrays
};

__global__ __launch_bounds__(MMI_SCORE_THREADS) void k_score_logprob(ScoreArgs a) {
    const int r = (int)blockIdx.x, s = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const uint16_t* row = a.logits + (long)s * a.site_stride + (long)r * a.ld;
    const long orow = (long)(r / a.F) * a.Tall + a.f0 + r % a.F;
    const int pieces = a.N / 8;
    const int tgt = a.targets[(long)r * a.tgt_stride + a.tgt_off + s];
    u32x4 v[MMI_SCORE_PIECES];
#pragma unroll
    for (int j = 0; j < MMI_SCORE_PIECES; ++j) {
        const int c = tid + j * MMI_SCORE_THREADS;
        v[j] = u32x4{0u, 0u, 0u, 0u};
        if (c < pieces) v[j] = *reinterpret_cast<const u32x4*>(row + 8 * c);
    }
    float* wide = a.lf32 ? a.lf32 + orow * a.lf32_row + (long)s * a.lf32_site : nullptr;
    float mx = -INFINITY, xt = 0.f;
    int mi = 0x7fffffff;
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
            if (wide) {
                *reinterpret_cast<f32x4*>(wide + 8 * c) = f32x4{f[0], f[1], f[2], f[3]};
                *reinterpret_cast<f32x4*>(wide + 8 * c + 4) = f32x4{f[4], f[5], f[6], f[7]};
            }
        }
    }
    // ---- the maximum and its lowest index: fixed tree
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float om = mmi_shfl_xor(mx, m);
        const int oi = mmi_shfl_xor(mi, m);
        if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; }
    }
    MMI_SHARED float s_mx[4];
    MMI_SHARED int s_mi[4];
    MMI_SHARED float s_sum[4];
    MMI_SHARED float s_xt;
    if (lane == 0) { s_mx[wave] = mx; s_mi[wave] = mi; }
    const bool has_t = tgt >= 0 && tgt < a.N;
    if (has_t && ((tgt >> 3) & (MMI_SCORE_THREADS - 1)) == tid) s_xt = xt;       // the thread that owns the token's piece
    __syncthreads();
    mx = s_mx[0]; mi = s_mi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_mx[w] > mx || (s_mx[w] == mx && s_mi[w] < mi)) { mx = s_mx[w]; mi = s_mi[w]; }
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
    if (tid == 0) {
        const float tot = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        const long o = orow * a.out_stride + a.out_off + s;
        a.logp[o] = has_t ? (s_xt - mx) - logf(tot) : -INFINITY;
        if (a.argmax) a.argmax[o] = mi == 0x7fffffff ? 0 : mi;
    }
}
