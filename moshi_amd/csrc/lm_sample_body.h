// The body of the two sampler kernels of lm_kernels.h, included once into each: k_sample (NUC = false: the sampler as it always
// was - every nucleus line sits behind `if constexpr (NUC)` or a constant-false `nuc`, and the kernel's text is otherwise the one it
// had as a plain kernel, so that its device code does not move) and k_sample_nucleus (NUC = true).  In scope: the template
// parameters NT and E, constexpr bool CACHE and NUC, and the kernel argument `SampleArgs a`.  No include guard on purpose.
    const int b = blockIdx.x, tid = threadIdx.x;
    MMI_SAMPLE_STAMP(0)
    const uint16_t* lg = a.logits + (long)b * a.ld;
    const int V = a.V;
    MMI_SHARED float redf[NT / 64];
    MMI_SHARED int redi[NT / 64];
    MMI_SHARED int redr[NT / 64];
    MMI_SHARED int hist[256];
    MMI_SHARED int wsum[NT / 64 + 1];
    MMI_SHARED float sel_val[256];
    MMI_SHARED __attribute__((aligned(16))) unsigned sel_cmp[256];   // (key << 16) | (0xffff - index): larger = earlier rank
    MMI_SHARED int sel_idx[256];
    MMI_SHARED int s_bin;
    MMI_SHARED int s_want;
    MMI_SHARED unsigned redk[NT / 64];
    MMI_SHARED unsigned wcnt[NT / 64][4];
    MMI_SHARED int s_rep[MMI_TEXT_HIST];     // the newest text tokens of an active row (repetition penalty)
    const int lane = tid & 63, wave = tid >> 6;
    const int i0 = tid * E;
    constexpr int NV = E / 8;
    // the step's control words, requested together with the logits: each is a memory round trip of its own where it is first
    // read otherwise (the RNG words in the middle of the scoring, the forcing words behind the last barrier: ~2 us of an 8 us kernel)
    const int g_use_noise = *a.use_noise;
    const unsigned long long g_seed = a.rng[0], g_step = a.rng[1];
    const int c_forced = *a.use_forced ? a.forced[(long)b * a.forced_stride] : -1;
    // the session's entry of the per-row table and its stream offset ride with them (workgroup-uniform: one row, one entry)
    const RowSamp c_row = a.rows[b];
    const long c_off = a.offsets[b];
    float c_top_p = 0.f;
    if constexpr (NUC) {
        const RowTopP tp = reinterpret_cast<const RowTopP*>(a.rows + a.B)[b];
        c_top_p = a.text ? tp.top_p_text : tp.top_p;
    }

    u32x4 cache[CACHE ? NV : 1];
    if constexpr (CACHE) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            cache[v] = u32x4{0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};      // bf16 -inf
            if (i0 + v * 8 < V) cache[v] = *reinterpret_cast<const u32x4*>(lg + i0 + v * 8);
        }
    }
    // visit the thread's entries: BODY sees `i` (vocabulary index, < V) and `bits` (the bf16 logit)
#define MMI_S_FOREACH(BODY)                                                                        \
    {                                                                                              \
        _Pragma("unroll") for (int v_ = 0; v_ < NV; ++v_) {                                        \
            if (i0 + v_ * 8 >= V) break;                                                           \
            u32x4 r4_;                                                                             \
            if constexpr (CACHE) r4_ = cache[v_];                                                  \
            else r4_ = *reinterpret_cast<const u32x4*>(lg + i0 + v_ * 8);                          \
            _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {                                     \
                const int i = i0 + v_ * 8 + e_;                                                    \
                const uint16_t bits = (uint16_t)((e_ & 1) ? (r4_[e_ >> 1] >> 16) : (r4_[e_ >> 1] & 0xffffu)); \
                BODY                                                                               \
            }                                                                                      \
        }                                                                                          \
    }

    // the same, skipping the thread's 8-entry vectors for which SKIP (an expression in v_) holds - the production path keeps the
    // largest key of each vector (vmax) and most vectors of a large vocabulary lie wholly under the top-k threshold
#define MMI_S_FOREACH_UNLESS(SKIP, BODY)                                                           \
    {                                                                                              \
        _Pragma("unroll") for (int v_ = 0; v_ < NV; ++v_) {                                        \
            if (i0 + v_ * 8 >= V) break;                                                           \
            if (SKIP) continue;                                                                    \
            u32x4 r4_;                                                                             \
            if constexpr (CACHE) r4_ = cache[v_];                                                  \
            else r4_ = *reinterpret_cast<const u32x4*>(lg + i0 + v_ * 8);                          \
            _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {                                     \
                const int i = i0 + v_ * 8 + e_;                                                    \
                const uint16_t bits = (uint16_t)((e_ & 1) ? (r4_[e_ >> 1] >> 16) : (r4_[e_ >> 1] & 0xffffu)); \
                BODY                                                                               \
            }                                                                                      \
        }                                                                                          \
    }

    // the same inside the nucleus select's window loop: the cached words pass through MMI_OPAQUE_U32, so that what is computed from
    // them (keys, high bytes, histogram addresses, probabilities: none changes from round to round) is computed where it is used and
    // not for all E entries ahead of the loop - that does not fit the 128 registers of a 1024-thread workgroup
#define MMI_S_FOREACH_ROUND(SKIP, BODY)                                                            \
    {                                                                                              \
        _Pragma("unroll") for (int v_ = 0; v_ < NV; ++v_) {                                        \
            if (i0 + v_ * 8 >= V) break;                                                           \
            if (SKIP) continue;                                                                    \
            u32x4 r4_ = cache[v_];                                                                 \
            _Pragma("unroll") for (int w_ = 0; w_ < 4; ++w_) { unsigned o_ = r4_[w_]; MMI_OPAQUE_U32(o_); r4_[w_] = o_; } \
            _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {                                     \
                const uint16_t bits = (uint16_t)((e_ & 1) ? (r4_[e_ >> 1] >> 16) : (r4_[e_ >> 1] & 0xffffu)); \
                BODY                                                                               \
            }                                                                                      \
        }                                                                                          \
    }

    // ---- the row's settings: its own entry when active, else the handle's (today's bits: global seed, counter (rng[1], site * B + b))
    const bool act = c_row.active != 0;
    const int s_use_sampling = act ? c_row.use_sampling : a.use_sampling;
    const float s_temp = act ? (a.text ? c_row.temp_text : c_row.temp) : a.temp;
    int s_k = act ? (a.text ? c_row.top_k_text : c_row.top_k) : a.k;
    if (s_k >= V || s_k > 256) s_k = 0;              // top_k == 0 (or the whole vocabulary): the full multinomial
    const int c_use_noise = act ? 0 : g_use_noise;   // supplied noise is a parity aid of the handle's settings (mmi_lm_step refuses it)
    const unsigned long long c_seed = act ? c_row.seed : g_seed, c_step = act ? (unsigned long long)c_off : g_step;
    const unsigned c_pa = act ? (unsigned)a.site : (unsigned)(a.site * a.B + b);
    const bool s_greedy = !s_use_sampling || !(s_temp > 0.f);
    // top_p > 0 overrides the site's top_k (sampling.py:97-98); greedy rows ignore it.  The draws are the device's own.
    const bool nuc = NUC && c_top_p > 0.f && !s_greedy;

    if constexpr (CACHE) {
        // the TTS machine's padding bonus (tts.py:553-555), where on_text_logits_hook runs: behind the guidance mix, ahead of the
        // repetition penalty.  bf16(float(l_pad) + bonus), the bits of the reference's in-place `+=` on its bf16 logits; like
        // that `+=` it is visible afterwards: the owning thread stores the entry back (the text-logits tap shows it).
        if (a.bonus != 0.f && a.bonus_id >= 0 && a.bonus_id < V && (unsigned)(a.bonus_id - i0) < (unsigned)E) {
            mmi_sample_patch<NV>(cache, a.bonus_id - i0, 1, a.bonus);
            const_cast<uint16_t*>(lg)[a.bonus_id] = mmi_sample_peek<NV>(cache, a.bonus_id - i0);
        }
        if (act && a.thist) {             // text site of an active row (block-uniform)
            const int have = c_row.hist_n < (unsigned)MMI_TEXT_HIST ? (int)c_row.hist_n : MMI_TEXT_HIST;
            int ctx = c_row.rep_context < have ? c_row.rep_context : have;
            if (ctx > MMI_TEXT_HIST) ctx = MMI_TEXT_HIST;
            if (ctx > 0 && c_row.rep_penalty != 1.f) {
                // newest first: slot (hist_n - 1 - j) % 64
                if (tid < ctx) s_rep[tid] = a.thist[(long)b * MMI_TEXT_HIST + (int)((c_row.hist_n - 1u - (unsigned)tid) & (unsigned)(MMI_TEXT_HIST - 1))];
                __syncthreads();
                for (int j = 0; j < ctx; ++j) {
                    const int t = s_rep[j];
                    if (t < 0 || t >= V || (unsigned)(t - i0) >= (unsigned)E) continue;      // not this thread's entry (or outside the vocabulary)
                    bool seen = false;
                    for (int jj = 0; jj < j; ++jj) seen = seen || s_rep[jj] == t;            // a token seen twice is penalised once
                    if (!seen) mmi_sample_patch<NV>(cache, t - i0, 0, c_row.rep_penalty);
                }
            }
            if (!s_greedy && c_row.pad_mult != 0.f && a.pad_id >= 0 && a.pad_id < V && (unsigned)(a.pad_id - i0) < (unsigned)E)
                mmi_sample_patch<NV>(cache, a.pad_id - i0, 1, c_row.pad_mult * s_temp);      // the fp32 product; the sum is the patch
        }
    }

    if (s_greedy) {
        // torch.argmax(logits): first maximum
        float best = -INFINITY;
        int bi = 0x7fffffff;
        MMI_S_FOREACH({
            const float v = mmi_bf16_to_f32(bits);
            if (v > best || bi == 0x7fffffff) { best = v; bi = i; }
        })
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            float ov = mmi_shfl_xor(best, m);
            int oi = mmi_shfl_xor(bi, m);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { redf[wave] = best; redi[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NT / 64; ++w)
                if (redf[w] > best || (redf[w] == best && redi[w] < bi)) { best = redf[w]; bi = redi[w]; }
            bi = mmi_apply_forced(a, b, bi);
            a.out[(long)b * a.out_stride] = bi;
            redi[0] = bi;
        }
        if (a.nx_out) {
            __syncthreads();
            mmi_sample_next_input(a, b, redi[0]);
        }
        return;
    }

    // The production path (top-k, on-device RNG): argmax_i p_i / q_i over the top-k set does not need the softmax at all -
    // log(p_i / q_i) = logit_i / temp - log q_i + const - and with no recorded draws to replay the Exp(1) draw of an entry may
    // be indexed by the entry instead of by its rank in the sorted top-k (i.i.d. draws assigned independently of their values:
    // the same distribution, checked by the frequency test the reference uses for its own sampler, sampling.py:109-127).  That
    // removes the two softmax passes, the ordered compaction and the rank computation from the critical path of every
    // sampling site; what stays is the radix select of the k-th largest logit.  Supplied noise (the parity taps) keeps the
    // reference's rank-indexed form below.
    const bool fast = (s_k > 0 && c_use_noise == 0) || nuc;
    float mx = -INFINITY, sum = 1.f;
    if (!fast || nuc) {
    // ---- softmax statistics of logits / temp (fp32)
    MMI_S_FOREACH({ mx = fmaxf(mx, mmi_bf16_to_f32(bits) / s_temp); })
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, mmi_shfl_xor(mx, m));
    if (lane == 0) redf[wave] = mx;
    __syncthreads();
    mx = redf[0];
    for (int w = 1; w < NT / 64; ++w) mx = fmaxf(mx, redf[w]);
    __syncthreads();
    sum = 0.f;
    MMI_S_FOREACH({ sum += expf(mmi_bf16_to_f32(bits) / s_temp - mx); })
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += mmi_shfl_xor(sum, m);
    if (lane == 0) redf[wave] = sum;
    __syncthreads();
    sum = 0.f;
    for (int w = 0; w < NT / 64; ++w) sum += redf[w];
    __syncthreads();
    }

    if (s_k <= 0 && !nuc) {
        // top_k = 0: `multinomial(probs)` over the whole vocabulary (sampling.py:98-106 without top-k/top-p): the reference
        // draws one Exp(1) per VOCABULARY ENTRY and takes argmax(p / q) (sampling.py:40-47); here the draw of entry i is the
        // counter RNG at (site, session, i).  Supplied noise (the parity taps) only exists for the top-k form.
        float score = -INFINITY;
        int tok = 0x7fffffff;
        MMI_S_FOREACH({
            const float pr = expf(mmi_bf16_to_f32(bits) / s_temp - mx) / sum;
            const float sc_ = pr / mmi_exp_noise(c_seed, c_step, c_pa, (unsigned)i);
            if (sc_ > score || (sc_ == score && i < tok)) { score = sc_; tok = i; }
        })
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float os = mmi_shfl_xor(score, m);
            const int ot = mmi_shfl_xor(tok, m);
            if (os > score || (os == score && ot < tok)) { score = os; tok = ot; }
        }
        if (lane == 0) { redf[wave] = score; redi[wave] = tok; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NT / 64; ++w)
                if (redf[w] > score || (redf[w] == score && redi[w] < tok)) { score = redf[w]; tok = redi[w]; }
            tok = mmi_apply_forced(a, b, tok);
            a.out[(long)b * a.out_stride] = tok;
            redi[0] = tok;
        }
        if (a.nx_out) {
            __syncthreads();
            mmi_sample_next_input(a, b, redi[0]);
        }
        return;
    }

    const int k = s_k < V ? s_k : V;
    int want = k;
    unsigned Tkey = 0u;
    // ---- production path (round 6): the k-th largest key WITHOUT the two 256-bin LDS histograms over every entry.  The logits of
    // a head share a handful of exponents, so the first histogram is 2048 (text head: 32000) LDS atomics on two or three
    // addresses - serialised - and each pass costs six workgroup barriers.  Instead: the block's largest key, then per-thread
    // PRIVATE counts (8 bits each, packed in 64) of the 8 high bytes at and below it, summed over the wave by shuffles and over
    // the waves through 16 words of LDS; the high byte that holds the k-th largest key is then known to every thread, and only
    // the entries carrying it (typically a few hundred, spread over the low byte's 256 bins) go through an LDS histogram, which
    // every wave scans for itself.  Three barriers instead of twelve.  A set that reaches below those 8 high bytes (more than
    // 2^16 in magnitude under the maximum: never with trained or random-init heads) falls through to the generic select below.
    bool have_t = false;
    int cnt_at_t = -1;                   // entries equal to the threshold key (window select only)
    unsigned vmax[NV];                   // largest key of each of the thread's vectors (production path)
#pragma unroll
    for (int v = 0; v < NV; ++v) vmax[v] = 0xffffu;
    if (fast) {
        unsigned km = 0u;
#pragma unroll
        for (int v = 0; v < NV; ++v) vmax[v] = 0u;
        MMI_S_FOREACH({ const unsigned ky = mmi_bf16_key(bits); vmax[v_] = ky > vmax[v_] ? ky : vmax[v_]; })
#pragma unroll
        for (int v = 0; v < NV; ++v) km = vmax[v] > km ? vmax[v] : km;
        km = mmi_wave_max_u32(km);
        if (lane == 0) redk[wave] = km;
        for (int j = tid; j < 256; j += NT) hist[j] = 0;
        MMI_SAMPLE_STAMP(1)
        __syncthreads();
        MMI_SAMPLE_STAMP(2)
        km = redk[0];
        for (int w = 1; w < NT / 64; ++w) km = redk[w] > km ? redk[w] : km;
        const int hi_max = (int)(km >> 8);
        if constexpr (NUC) if (nuc) {
            // ---- the nucleus as (Tkey, want_eq): the mass-weighted form of the select below.  P(entry) = softmax(x / temp) with the
            // mx / sum above.  Per window of 8 high bytes: private per-thread masses, butterfly over the wave, waves summed in wave
            // order - the same bits under every schedule.  The high byte that holds the boundary goes through the integer histogram
            // of its low bytes; the mass of a bin is count * P(key).  A boundary under the window: the window moves down to the next
            // high byte that holds an entry (zero-centred logits leave the bytes of the tiny magnitudes, between the positive and the
            // negative values, empty) and the mass found so far carries over (at most 32 rounds).
            MMI_SHARED float wmass[NT / 64][8];
            MMI_SHARED unsigned wnext[NT / 64];
            const float p = c_top_p;
            if (p >= 1.f) { Tkey = 0u; want = V; have_t = true; }          // the whole vocabulary
            float carry = 0.f;
            for (int hi_top = hi_max; !have_t;) {                          // block-uniform
                float m8[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) m8[q] = 0.f;
                unsigned below = 0u;                                       // 1 + the largest high byte under the window that holds an entry
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    if (i0 + v * 8 < V && (int)(vmax[v] >> 8) < hi_top - 7) below = (vmax[v] >> 8) + 1u > below ? (vmax[v] >> 8) + 1u : below;
                // One entry at a time, fenced, on copies of temp and mx the compiler cannot see through: it would otherwise keep every
                // entry's expf and division in flight at once, or compute all E probabilities ahead of the window loop (they do not
                // change from round to round) - neither fits the 128 registers of a 1024-thread workgroup next to the cached logits.
                float r_temp = s_temp, r_mx = mx;
                MMI_OPAQUE_F32(r_temp);
                MMI_OPAQUE_F32(r_mx);
                MMI_S_FOREACH_ROUND((int)(vmax[v_] >> 8) < hi_top - 7, {
                    const int d = hi_top - (int)(mmi_bf16_key(bits) >> 8);
                    if ((unsigned)d < 8u) {
                        const float pr = expf(mmi_bf16_to_f32(bits) / r_temp - r_mx) / sum;
                        _Pragma("unroll") for (int q = 0; q < 8; ++q) m8[q] += d == q ? pr : 0.f;
                    } else if (d >= 8) below = (unsigned)(hi_top - d) + 1u > below ? (unsigned)(hi_top - d) + 1u : below;
                    MMI_SCHED_FENCE();
                })
#pragma unroll
                for (int q = 0; q < 8; ++q) {
#pragma unroll
                    for (int m = 32; m >= 1; m >>= 1) m8[q] += mmi_shfl_xor(m8[q], m);
                    if (lane == 0) wmass[wave][q] = m8[q];
                }
                below = mmi_wave_max_u32(below);
                if (lane == 0) wnext[wave] = below;
                __syncthreads();
                for (int w = 0; w < NT / 64; ++w) below = wnext[w] > below ? wnext[w] : below;
#pragma unroll
                for (int q = 0; q < 8; ++q) m8[q] = 0.f;
#pragma unroll 1
                for (int w = 0; w < NT / 64; ++w)                          // the waves in wave order
#pragma unroll
                    for (int q = 0; q < 8; ++q) m8[q] += wmass[w][q];
                float A = carry;                                           // mass of every high byte above the candidate
                int dsel = -1;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float nx = A + m8[q];
                    if (dsel < 0) { if (nx > p) dsel = q; else A = nx; }
                }
                __syncthreads();
                if (dsel < 0) {
                    carry = A;
                    if (below == 0u) { Tkey = 0u; want = V; have_t = true; }      // nothing under the window: the mass never passed p
                    hi_top = (int)below - 1;
                    continue;
                }
                const unsigned hi_sel = (unsigned)(hi_top - dsel);        // holds an entry: its mass is > 0
                MMI_S_FOREACH_ROUND((vmax[v_] >> 8) < hi_sel, {
                    const unsigned ky = mmi_bf16_key(bits);
                    if ((ky >> 8) == hi_sel) mmi_atomic_add(reinterpret_cast<unsigned*>(&hist[ky & 255u]), 1u);
                })
                __syncthreads();
                // every wave for itself: lane l looks at bins 255 - 4l .. 252 - 4l (descending keys)
                int c4[4];
                float p4[4], m4[4], s4 = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int bin = 255 - 4 * lane - j;
                    c4[j] = hist[bin];
                    p4[j] = expf(mmi_bf16_to_f32(mmi_bf16_unkey((hi_sel << 8) | (unsigned)bin)) / s_temp - mx) / sum;
                    m4[j] = c4[j] > 0 ? (float)c4[j] * p4[j] : 0.f;
                    s4 += m4[j];
                    MMI_SCHED_FENCE();
                }
                float inc = s4;
#pragma unroll
                for (int dlt = 1; dlt < 64; dlt <<= 1) {
                    const float o = mmi_shfl(inc, lane - dlt);
                    if (lane >= dlt) inc += o;
                }
                const float before = mmi_shfl(inc, lane - 1);
                float run = A + (lane > 0 ? before : 0.f);                 // mass above the lane's first bin
                // the lowest bin that holds an entry whose preceding mass is <= p
                int tb = 256, tc = 0;
                float ta = 0.f, tp = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (c4[j] > 0 && run <= p) { tb = 255 - 4 * lane - j; tc = c4[j]; ta = run; tp = p4[j]; }
                    run += m4[j];
                }
                int bmin = tb;
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) { const int o = mmi_shfl_xor(bmin, m); bmin = o < bmin ? o : bmin; }
                if (bmin > 255) { Tkey = hi_sel << 8; want = V; have_t = true; continue; }   // (cannot be: the byte's first entry qualifies)
                const int src = (255 - bmin) >> 2;                         // the lane whose lowest qualifying bin it is
                tc = mmi_shfl(tc, src); ta = mmi_shfl(ta, src); tp = mmi_shfl(tp, src);
                // entry j of the bin (index order) is in iff ta + j * tp <= p: j = 0 is; the count by bisection (monotone in j)
                int lo = 0, hi = tc;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (ta + (float)mid * tp <= p) lo = mid; else hi = mid;
                }
                Tkey = (hi_sel << 8) | (unsigned)bmin;
                want = lo + 1;
                cnt_at_t = tc;
                have_t = true;
            }
        }
        if (!nuc) {
        unsigned long long pc = 0ull;
        MMI_S_FOREACH({
            const int d = hi_max - (int)(mmi_bf16_key(bits) >> 8);
            if (d < 8) pc += 1ull << (8 * d);
        })
        // 8 x 8-bit counters (<= E <= 32 each) -> 4 words of two 16-bit fields: wave sums <= 64 * 32, block sums <= NT * E <= 32768
        unsigned f[4] = {(unsigned)pc & 0x00ff00ffu, ((unsigned)pc >> 8) & 0x00ff00ffu, (unsigned)(pc >> 32) & 0x00ff00ffu, ((unsigned)(pc >> 32) >> 8) & 0x00ff00ffu};
#pragma unroll
        for (int q = 0; q < 4; ++q) f[q] = mmi_wave_sum_u32(f[q]);
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < 4; ++q) wcnt[wave][q] = f[q];
        MMI_SAMPLE_STAMP(3)
        __syncthreads();
        MMI_SAMPLE_STAMP(4)
        unsigned t4[4] = {0u, 0u, 0u, 0u};
        for (int w = 0; w < NT / 64; ++w)
#pragma unroll
            for (int q = 0; q < 4; ++q) t4[q] += wcnt[w][q];
        // counter d of the packed word: byte d -> word (d >> 2) * 2 + (d & 1), field (d >> 1) & 1
        int cum = 0, dsel = -1, want1 = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const unsigned wq = t4[(d >> 2) * 2 + (d & 1)];
            const int c = (int)(((d >> 1) & 1) ? (wq >> 16) : (wq & 0xffffu));
            if (dsel < 0 && cum + c >= k) { dsel = d; want1 = k - cum; }
            cum += c;
        }
        if (dsel >= 0 && hi_max - dsel >= 0) {                     // block-uniform
            const unsigned hi_sel = (unsigned)(hi_max - dsel);
            MMI_S_FOREACH_UNLESS((vmax[v_] >> 8) < hi_sel, {
                const unsigned ky = mmi_bf16_key(bits);
                if ((ky >> 8) == hi_sel) mmi_atomic_add(reinterpret_cast<unsigned*>(&hist[ky & 255u]), 1u);
            })
            MMI_SAMPLE_STAMP(5)
            __syncthreads();
            MMI_SAMPLE_STAMP(6)
            // every wave for itself: lane l looks at bins 255 - 4l .. 252 - 4l (descending keys); `above` = entries in higher bins
            int c4[4], s4 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c4[j] = hist[255 - 4 * lane - j]; s4 += c4[j]; }
            int inc = s4;
#pragma unroll
            for (int dlt = 1; dlt < 64; dlt <<= 1) {
                const int o = mmi_shfl(inc, lane - dlt);
                if (lane >= dlt) inc += o;
            }
            int run = inc - s4, fb = 0, fw = 0, fc = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (run < want1 && want1 <= run + c4[j]) { fb = 256 - 4 * lane - j; fw = want1 - run; fc = c4[j]; }   // exactly one (lane, j)
                run += c4[j];
            }
            {   // the finder's values are the only non-zero ones: a sum over the wave hands them to every lane
                const unsigned p0 = mmi_wave_sum_u32((unsigned)fb | ((unsigned)fw << 16)), p1 = mmi_wave_sum_u32((unsigned)fc);
                fb = (int)(p0 & 0xffffu); fw = (int)(p0 >> 16); fc = (int)p1;
            }
            Tkey = (hi_sel << 8) | (unsigned)(fb - 1);
            want = fw;
            cnt_at_t = fc;
            have_t = true;
        }
        }
    }
    // ---- radix select of the k-th largest key: high byte, then low byte (supplied noise: the parity taps; and the fallback)
    for (int pass = 0; pass < 2 && !have_t; ++pass) {
        for (int j = tid; j < 256; j += NT) hist[j] = 0;
        __syncthreads();
        MMI_S_FOREACH({
            const unsigned ky = mmi_bf16_key(bits);
            if (pass == 0 || (ky >> 8) == (Tkey >> 8))
                mmi_atomic_add(reinterpret_cast<unsigned*>(&hist[pass == 0 ? (ky >> 8) : (ky & 255u)]), 1u);
        })
        __syncthreads();
        {   // bin holding the want-th largest key: thread t looks at bin 255-t; `above` = entries in higher bins
            const int bin = 255 - tid;
            const int cnt = tid < 256 ? hist[bin] : 0;
            int total;
            const int above = mmi_block_excl_scan<NT>(cnt, wsum, &total);
            if (tid < 256 && above < want && want <= above + cnt) { s_bin = bin; s_want = want - above; }
        }
        __syncthreads();
        Tkey |= (unsigned)s_bin << (pass == 0 ? 8 : 0);
        want = s_want;
        __syncthreads();
    }
    const int want_eq = want;          // how many entries equal to the threshold belong to the set (lowest indices first)
    MMI_SAMPLE_STAMP(7)

    // ---- ordered compaction of the top-k set (index order)
    int n_gt = 0, n_eq = 0;
    MMI_S_FOREACH_UNLESS(vmax[v_] < Tkey, {
        const unsigned ky = mmi_bf16_key(bits);
        n_gt += ky > Tkey ? 1 : 0;
        n_eq += ky == Tkey ? 1 : 0;
    })
    int tot = 0;
    int eq_take = n_eq;                // window select and every entry at the threshold belongs to the set: no scan (block-uniform)
    if (!(have_t && cnt_at_t == want_eq)) {
        const int eq_base = mmi_block_excl_scan<NT>(n_eq, wsum, &tot);
        eq_take = want_eq - eq_base;
        eq_take = eq_take < 0 ? 0 : (eq_take > n_eq ? n_eq : eq_take);
    }
    MMI_SAMPLE_STAMP(8)
    if (fast) {
        // every member of the set scores logit / temp - log(q), q ~ Exp(1); the largest wins.  One Philox4x32-10 call serves the
        // four entries 4j .. 4j + 3 of the vocabulary (counter (step, site * B + session, j), one output word each) and is skipped
        // when none of the four is in the set: two calls per thread for an audio head instead of eight, ~one for the text head
        float best = -INFINITY;
        int bi = 0x7fffffff;
        int eq_seen_f = 0;
        const float inv_t = 1.0f / s_temp;
        const unsigned long long seed = c_seed, step = c_step;
#pragma unroll
        for (int v_ = 0; v_ < NV; ++v_) {
            if (i0 + v_ * 8 >= V) break;
            if (vmax[v_] < Tkey) continue;          // no member of the set in this vector
            u32x4 r4_;
            if constexpr (CACHE) r4_ = cache[v_];
            else r4_ = *reinterpret_cast<const u32x4*>(lg + i0 + v_ * 8);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                bool tk[4];
                bool any = false;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int e_ = 4 * h + e;
                    const uint16_t bits = (uint16_t)((e_ & 1) ? (r4_[e_ >> 1] >> 16) : (r4_[e_ >> 1] & 0xffffu));
                    const unsigned ky = mmi_bf16_key(bits);
                    bool take = ky > Tkey;
                    if (ky == Tkey) { take = eq_seen_f < eq_take; ++eq_seen_f; }
                    tk[e] = take;
                    any = any || take;
                }
                if (!any) continue;
                unsigned r[4];
                mmi_philox4(seed, step, c_pa, (unsigned)((i0 + v_ * 8 + 4 * h) >> 2), r);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!tk[e]) continue;
                    const int e_ = 4 * h + e, i = i0 + v_ * 8 + e_;
                    const uint16_t bits = (uint16_t)((e_ & 1) ? (r4_[e_ >> 1] >> 16) : (r4_[e_ >> 1] & 0xffffu));
                    const float u = fminf(((float)(r[e] >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);   // (0, 1): see mmi_exp_noise
                    const float sc_ = mmi_bf16_to_f32(bits) * inv_t - mmi_fast_logf(-mmi_fast_logf(u));
                    if (sc_ > best || (sc_ == best && i < bi)) { best = sc_; bi = i; }
                }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ob = mmi_shfl_xor(best, m);
            const int oi = mmi_shfl_xor(bi, m);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        MMI_SAMPLE_STAMP(9)
        if (lane == 0) { redf[wave] = best; redi[wave] = bi; }
        __syncthreads();
        MMI_SAMPLE_STAMP(10)
        // only the threads that write the next micro-step's input row (and thread 0, for the token) go on: a 1024-thread workgroup
        // would otherwise run this tail sixteen times over on its four SIMDs
        if (tid != 0 && (!a.nx_out || tid >= (a.nx_dup ? 2 : 1) * (a.nx_D / 8))) return;
        best = redf[0]; bi = redi[0];                   // every remaining thread folds the waves' winners itself: no second barrier
        for (int w = 1; w < NT / 64; ++w)
            if (redf[w] > best || (redf[w] == best && redi[w] < bi)) { best = redf[w]; bi = redi[w]; }
        bi = c_forced >= 0 ? c_forced : bi;            // (mmi_apply_forced, on the words requested at the top)
        if (tid == 0) a.out[(long)b * a.out_stride] = bi;
        MMI_SAMPLE_STAMP(11)
        mmi_sample_next_input(a, b, bi);
        MMI_SAMPLE_STAMP(12)
        return;
    }
    int pos = mmi_block_excl_scan<NT>(n_gt + eq_take, wsum, &tot);
    int eq_seen = 0;
    MMI_S_FOREACH({
        const unsigned ky = mmi_bf16_key(bits);
        bool take = ky > Tkey;
        if (ky == Tkey) { take = eq_seen < eq_take; ++eq_seen; }
        if (take) {
            if (pos < 256) {
                sel_val[pos] = expf(mmi_bf16_to_f32(bits) / s_temp - mx) / sum;
                sel_cmp[pos] = (ky << 16) | (unsigned)(0xffff - i);
                sel_idx[pos] = i;
            }
            ++pos;
        }
    })
#undef MMI_S_FOREACH
#undef MMI_S_FOREACH_UNLESS
#undef MMI_S_FOREACH_ROUND
    __syncthreads();
    // ---- rank inside the set (descending logit, then index) and the noisy argmax
    float score = -INFINITY;
    int rank = 0x7fffffff, tok = 0;
    for (int j = k + tid; j < 256; j += NT) sel_cmp[j] = 0u;      // entries past the set never outrank anything
    __syncthreads();
    if (tid < k && tid < 256) {
        const float v = sel_val[tid];
        const unsigned mine = sel_cmp[tid];
        const int id = sel_idx[tid];
        int r = 0;
        for (int m = 0; m < k; m += 4) {
            const u32x4 o = *reinterpret_cast<const u32x4*>(&sel_cmp[m]);
            r += (o[0] > mine ? 1 : 0) + (o[1] > mine ? 1 : 0) + (o[2] > mine ? 1 : 0) + (o[3] > mine ? 1 : 0);
        }
        float q;
        if (c_use_noise) q = a.noise[(long)b * a.noise_ld + r];
        else q = mmi_exp_noise(c_seed, c_step, c_pa, (unsigned)r);
        score = v / q;
        rank = r;
        tok = id;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        float os = mmi_shfl_xor(score, m);
        int orank = mmi_shfl_xor(rank, m), otok = mmi_shfl_xor(tok, m);
        if (os > score || (os == score && orank < rank)) { score = os; rank = orank; tok = otok; }
    }
    if (lane == 0) { redf[wave] = score; redi[wave] = tok; redr[wave] = rank; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NT / 64; ++w)
            if (redf[w] > score || (redf[w] == score && redr[w] < rank)) { score = redf[w]; rank = redr[w]; tok = redi[w]; }
        tok = mmi_apply_forced(a, b, tok);
        a.out[(long)b * a.out_stride] = tok;
        redi[0] = tok;
    }
    if (a.nx_out) {
        __syncthreads();
        mmi_sample_next_input(a, b, redi[0]);
    }
