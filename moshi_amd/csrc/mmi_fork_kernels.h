// Forking a live session into other slots of the same handle (mmi_lm_fork_session / mmi_mimi_fork_session):
// the two kernels both engines launch.
//   k_fork_ring  the valid prefix of every ring segment of the source session -> up to 16 destination sessions.  Used for the
//                LM's temporal ring (bf16, e4m3, and both planes of a 4-bit layer) and for the codec's two transformer rings.
//   k_fork_rows  the small per-session slices (offsets, token rings, sampling entries, conditions, conv histories, ...), one
//                launch per engine, by a descriptor list that rides in the kernel arguments.
// Neither kernel reads anything on the host's behalf: the valid length of a ring segment is read on the device, the host sizes
// the grid from a bound it already holds, and workgroups past the valid length exit.  No LDS, no atomics.  (The kernels are
// `static`: the header is compiled into both engines' objects.)
#pragma once
#include "mmi_common.h"

#define MMI_FORK_MAX_DST 16
#define MMI_FORK_THREADS 256
#define MMI_FORK_CHUNK 8192        // bytes of a ring segment per workgroup: two 16-byte loads in flight per thread
#define MMI_FORK_MAX_ENT 48

// The sessions of one call.  A session is `n_rows` model rows: b, and on a guided stream its twin b + twin.
struct ForkSessions {
    int src, n_dst, n_rows, twin;
    int dst[MMI_FORK_MAX_DST];
};

// `src` / `dst` of a fork call checked against a stream of `batch` sessions (include/moshi_mi.h: the refusals)
static inline int mmi_fork_sessions(const char* who, int batch, int32_t src, const int32_t* dst, int32_t n_dst, ForkSessions* out) {
    const std::string w(who);
    if (!dst) return mmi_fail(MMI_ERR_INVALID, w + ": null destination list");
    if (n_dst < 1 || n_dst > MMI_FORK_MAX_DST) return mmi_fail(MMI_ERR_INVALID, w + ": n_dst must be in [1, 16]");
    if (src < 0 || src >= batch) return mmi_fail(MMI_ERR_INVALID, w + ": src outside [0, batch)");
    memset(out, 0, sizeof(*out));
    out->src = src; out->n_dst = n_dst; out->n_rows = 1;
    for (int i = 0; i < n_dst; ++i) {
        if (dst[i] < 0 || dst[i] >= batch) return mmi_fail(MMI_ERR_INVALID, w + ": a destination outside [0, batch)");
        if (dst[i] == src) return mmi_fail(MMI_ERR_INVALID, w + ": a destination equals the source");
        for (int j = 0; j < i; ++j)
            if (dst[j] == dst[i]) return mmi_fail(MMI_ERR_INVALID, w + ": a destination is named twice");
        out->dst[i] = dst[i];
    }
    return MMI_OK;
}

// ------------------------------------------------------------------------------------------------
// the rings
// ------------------------------------------------------------------------------------------------
// A ring is `n_base` allocations (LM: keys, values; codec: one) of `layers` layers of `layer_stride` bytes; a layer holds
// `n_planes` planes (the 4-bit LM ring: codes, then scales at KvRing::scale_off), a plane is [row][head][cap] positions of
// pos_bytes[plane] bytes.  A (base, layer, plane, row, head) segment is contiguous, and positions [0, min(len[session], cap)) of
// it are the valid ones: the ring is written at position offset % cap, so after a wrap the whole segment is valid.
struct ForkRingArgs {
    uint8_t* base[2];
    long layer_stride;
    long plane_off[2];
    int pos_bytes[2];
    int vec[2];             // the plane's segments start 16-byte aligned (false at some tiny test shapes): 16-byte accesses
    int n_base, layers, n_planes, H, cap;
    int x0;                 // chunks of plane 0 by the host's bound (set by mmi_launch_fork_ring): the grid's x holds the planes' chunks
                            // one after the other, so the 8 x shorter scale plane of a 4-bit layer launches 8 x fewer workgroups
    const long* len;        // [sessions] positions written so far: the LM's offsets, or one of the codec's counters (a guided
                            // session's twin row is as deep as the session; offsets_m is the step's own copy and lags a step)
    ForkSessions s;
};

// grid (chunks of a segment by the host's bound, plane after plane; n_base * layers * n_rows * H segments).  Every source fragment is loaded
// once (non-temporal: it is not read again before the next step streams the ring anyway) and stored n_dst times.  Positions past
// the valid prefix of a destination keep their bytes: they hold finite values already, which is all the attention asks of them.
static __global__ __launch_bounds__(MMI_FORK_THREADS) void k_fork_ring(ForkRingArgs a) {
    int seg = (int)blockIdx.y;
    const int head = seg % a.H; seg /= a.H;
    const int r = seg % a.s.n_rows; seg /= a.s.n_rows;
    const int layer = seg % a.layers, which = seg / a.layers;
    const int plane = (int)blockIdx.x >= a.x0 ? 1 : 0;
    const int srow = a.s.src + r * a.s.twin;
    long valid = a.len[a.s.src];
    if (valid > (long)a.cap) valid = a.cap;
    const long bytes = valid * a.pos_bytes[plane];
    const long c0 = (long)((int)blockIdx.x - plane * a.x0) * MMI_FORK_CHUNK;
    if (c0 >= bytes) return;
    const long n = bytes - c0 < (long)MMI_FORK_CHUNK ? bytes - c0 : (long)MMI_FORK_CHUNK;
    const long seg_bytes = (long)a.cap * a.pos_bytes[plane];
    uint8_t* pb = a.base[which] + (long)layer * a.layer_stride + a.plane_off[plane] + (long)head * seg_bytes + c0;
    const long row_bytes = (long)a.H * seg_bytes;
    const uint8_t* src = pb + (long)srow * row_bytes;
    const long tid = (long)threadIdx.x;
    const long n16 = a.vec[plane] ? n / 16 : 0;
    const u32x4* s16 = reinterpret_cast<const u32x4*>(src);
    for (long i = tid; i < n16; i += 2 * MMI_FORK_THREADS) {
        const bool two = i + MMI_FORK_THREADS < n16;
        const u32x4 v0 = mmi_load_nt(s16 + i);
        const u32x4 v1 = two ? mmi_load_nt(s16 + i + MMI_FORK_THREADS) : v0;
        for (int j = 0; j < a.s.n_dst; ++j) {
            u32x4* d16 = reinterpret_cast<u32x4*>(pb + (long)(a.s.dst[j] + r * a.s.twin) * row_bytes);
            d16[i] = v0;
            if (two) d16[i + MMI_FORK_THREADS] = v1;
        }
    }
    for (long i = n16 * 16 + tid; i < n; i += MMI_FORK_THREADS) {      // the byte tail (a length that is no multiple of 16)
        const uint8_t v = src[i];
        for (int j = 0; j < a.s.n_dst; ++j) (pb + (long)(a.s.dst[j] + r * a.s.twin) * row_bytes)[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// the per-session rows
// ------------------------------------------------------------------------------------------------
// One buffer with per-session slices: session row b owns, for o in [0, outer), the `slice` bytes at
// p + o * outer_stride + b * row_stride.  (A plain [rows][slice] buffer: outer 1, row_stride = slice.  The LM's cross-attention
// source [layers][rows][slice]: outer = layers.  A conv history of the codec [rows][C][ld], the first H floats of every channel:
// outer = C, outer_stride = ld floats, row_stride = C * ld floats, slice = H floats.)
struct ForkEnt {
    uint8_t* p;
    long outer_stride, row_stride, slice;
    int outer;
    int twin;               // the buffer has a row per MODEL row: on a guided stream the twin row follows its session
    int unit;               // 16, 4 or 1: the widest access every slice's address and length allow
};
struct ForkRowArgs {
    ForkEnt e[MMI_FORK_MAX_ENT];
    int n;
    uint8_t* exec;          // exec[dst] = 1, as a reset leaves it (the source's own bit is not copied: a parked template has 0)
    ForkSessions s;
};

// false: the list is full (nothing was added)
static inline bool mmi_fork_add(ForkRowArgs& a, void* p, int outer, size_t outer_stride, size_t row_stride, size_t slice, bool twin) {
    if (a.n >= MMI_FORK_MAX_ENT) return false;
    ForkEnt& e = a.e[a.n++];
    e.p = reinterpret_cast<uint8_t*>(p);
    e.outer = outer; e.outer_stride = (long)outer_stride; e.row_stride = (long)row_stride; e.slice = (long)slice; e.twin = twin ? 1 : 0;
    const size_t all = (size_t)reinterpret_cast<uintptr_t>(p) | outer_stride | row_stride | slice;
    e.unit = all % 16 == 0 ? 16 : (all % 4 == 0 ? 4 : 1);
    return true;
}

// grid (workgroups striding over a session's bytes of the entry, entries, n_rows)
static __global__ __launch_bounds__(MMI_FORK_THREADS) void k_fork_rows(ForkRowArgs a) {
    const int r = (int)blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && r == 0 && (int)threadIdx.x < a.s.n_dst) a.exec[a.s.dst[threadIdx.x]] = 1;
    const ForkEnt e = a.e[blockIdx.y];
    if (r > 0 && !e.twin) return;
    const long srow = a.s.src + r * a.s.twin;
    const long units = (long)e.outer * e.slice / e.unit;
    for (long u = (long)blockIdx.x * MMI_FORK_THREADS + (long)threadIdx.x; u < units; u += (long)gridDim.x * MMI_FORK_THREADS) {
        const long byte = u * e.unit;
        const long o = byte / e.slice;
        uint8_t* at = e.p + o * e.outer_stride + (byte - o * e.slice);
        const uint8_t* src = at + srow * e.row_stride;
        if (e.unit == 16) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(src);
            for (int j = 0; j < a.s.n_dst; ++j) *reinterpret_cast<u32x4*>(at + (long)(a.s.dst[j] + r * a.s.twin) * e.row_stride) = v;
        } else if (e.unit == 4) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(src);
            for (int j = 0; j < a.s.n_dst; ++j) *reinterpret_cast<uint32_t*>(at + (long)(a.s.dst[j] + r * a.s.twin) * e.row_stride) = v;
        } else {
            const uint8_t v = *src;
            for (int j = 0; j < a.s.n_dst; ++j) at[(long)(a.s.dst[j] + r * a.s.twin) * e.row_stride] = v;
        }
    }
}

// The launch of k_fork_rows: the grid's x covers the largest entry (at most 64 workgroups: the rest strides)
static inline int mmi_launch_fork_rows(hipStream_t s, const ForkRowArgs& a) {
    long most = 1;
    for (int i = 0; i < a.n; ++i) {
        const long u = (long)a.e[i].outer * a.e[i].slice / a.e[i].unit;
        most = u > most ? u : most;
    }
    long gx = (most + MMI_FORK_THREADS - 1) / MMI_FORK_THREADS;
    gx = gx > 64 ? 64 : gx;
    MMI_LAUNCH(k_fork_rows, dim3((unsigned)gx, (unsigned)a.n, (unsigned)a.s.n_rows), MMI_FORK_THREADS, 0, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// The launch of k_fork_ring for a bound on the valid positions the host already holds (0: nothing to copy)
static inline int mmi_launch_fork_ring(hipStream_t s, ForkRingArgs a, long bound) {
    if (bound > (long)a.cap) bound = a.cap;
    if (bound <= 0) return MMI_OK;
    long gx = 0;
    for (int p = 0; p < a.n_planes; ++p) {
        if (p == 1) a.x0 = (int)gx;
        gx += (bound * a.pos_bytes[p] + MMI_FORK_CHUNK - 1) / MMI_FORK_CHUNK;
    }
    if (a.n_planes == 1) a.x0 = (int)gx;
    MMI_LAUNCH(k_fork_ring, dim3((unsigned)gx, (unsigned)(a.n_base * a.layers * a.s.n_rows * a.H)), MMI_FORK_THREADS, 0, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}
