// Where does the decode attention's time go?  k_lm_attn_wave<128> (lm_kernels.h, bf16 ring) at the flagship step's shape - 32 sessions
// x 32 heads, capacity 3000, ring depths 250 + 8 b (the benchmark's mid depth) and 500 + 8 b - as a dependent chain in one stream: a
// small kernel writes `qrot` and the newest ring row in front of every launch, so the query is cold as it is behind in_proj.
// Prints the time per launch, and the kernel's own stage stamps (MMI_ATTN_STAMP, the 100 MHz wall clock, thread 0 of every workgroup)
// reduced to min / median / max over the 1024 workgroups.  Measurement tool only.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Imoshi_amd/csrc scripts/attn_stamps.hip moshi_amd/csrc/api_common.hip -o build/attn_stamps
#include <hip/hip_runtime.h>
#define ATTN_NSTAMP 8
__device__ long long g_attn_stamps[1024 * ATTN_NSTAMP];
// The stamps stay in LDS until the output is stored: a global store would count on vmcnt like the ring's loads and move the waits.
__device__ __forceinline__ long long* attn_stamp_buf() { __shared__ long long s[ATTN_NSTAMP]; return s; }
// `dep`: a value the stage produces - the clock is read once it exists
#define MMI_ATTN_STAMP(i, dep) { asm volatile("" :: "v"(dep)); if (threadIdx.x == 0) attn_stamp_buf()[i] = (long long)wall_clock64(); }
// the first round has landed when no more loads are outstanding than the second round's (vector memory loads return in order)
#define MMI_ATTN_STAMP_LANDED(i, first) if (first) { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * NB * (KV4 ? 2 : 1)) : "memory"); if (threadIdx.x == 0) attn_stamp_buf()[i] = (long long)wall_clock64(); }
#define MMI_ATTN_STAMP_STORED(i) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (threadIdx.x == 0) { long long* s_ = attn_stamp_buf(); s_[i] = (long long)wall_clock64(); \
        for (int q_ = 0; q_ < ATTN_NSTAMP; ++q_) g_attn_stamps[(size_t)blockIdx.x * ATTN_NSTAMP + q_] = s_[q_]; } }
#include "lm_kernels.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

__global__ void k_fill_bf16(uint16_t* p, size_t n, unsigned seed) {        // values in (-1, 1)
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        unsigned h = (unsigned)(i * 2654435761u) ^ seed;
        h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
        p[i] = mmi_f32_to_bf16((float)(h & 0xffff) / 32768.0f - 1.0f);
    }
}
// the "previous kernel" (in_proj's epilogue in the step): the roped query and the newest key / value row of every (session, head)
__global__ void k_touch(LmAttnArgs a, unsigned seed) {
    const int bh = blockIdx.x, d = threadIdx.x;        // 128 threads
    const long slot = a.offsets[bh / a.H] % a.cap;
    unsigned h = (unsigned)((bh * 128 + d) * 2654435761u) ^ seed;
    h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
    const uint16_t v = mmi_f32_to_bf16((float)(h & 0xffff) / 32768.0f - 1.0f);
    a.qrot[(long)bh * 128 + d] = v;
    a.kc[((long)bh * a.cap + slot) * 128 + d] = v;
    a.vc[((long)bh * a.cap + slot) * 128 + d] = v;
}

template <class F>
double chain_us(hipStream_t s, int n, F launch) {
    hipGraph_t g; hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < n; ++i) launch(i);
    CK(hipStreamEndCapture(s, &g));
    CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipGraphLaunch(ge, s)); CK(hipStreamSynchronize(s));
    CK(hipEventRecord(e0, s));
    for (int r = 0; r < 5; ++r) CK(hipGraphLaunch(ge, s));
    CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
    return 1e3 * ms / (5.0 * n);
}

int main() {
    hipStream_t s; CK(hipStreamCreate(&s));
    const int B = 32, H = 32, DH = 128, cap = 3000, n = 100, NBH = B * H;
    const size_t ring = (size_t)NBH * cap * DH;
    LmAttnArgs a; memset(&a, 0, sizeof(a));
    long* offsets;
    CK(hipMalloc(&a.qrot, (size_t)NBH * DH * 2)); CK(hipMalloc(&a.kc, ring * 2)); CK(hipMalloc(&a.vc, ring * 2));
    CK(hipMalloc(&offsets, B * sizeof(long))); CK(hipMalloc(&a.out, (size_t)(H * DH / 16) * 512 * 2));
    a.offsets = offsets; a.B = B; a.H = H; a.Dh = DH; a.cap = cap; a.context = cap; a.NS = 1; a.T = 32; a.out_ksteps = H * DH / 16;
    a.solo_rows = -1;
    k_fill_bf16<<<4096, 256, 0, s>>>(a.kc, ring, 11u);
    k_fill_bf16<<<4096, 256, 0, s>>>(a.vc, ring, 23u);
    CK(hipStreamSynchronize(s));
    static const char* stage[] = {"entry", "offset returned", "first round landed", "last round used", "slots merged", "waves merged", "stored"};
    for (int base : {250, 500}) {
        long ho[B]; double bytes = 0;
        for (int b = 0; b < B; ++b) { ho[b] = base + 8 * b - 1; bytes += (double)(ho[b] + 1) * H * DH * 2 * 2; }
        CK(hipMemcpy(offsets, ho, sizeof(ho), hipMemcpyHostToDevice));
        const double t = chain_us(s, n, [&](int i) {
            hipLaunchKernelGGL(k_touch, dim3(NBH), dim3(128), 0, s, a, (unsigned)i);
            hipLaunchKernelGGL((k_lm_attn_wave<128>), dim3(NBH, 1), dim3(256), 0, s, a);
        });
        const double t0 = chain_us(s, n, [&](int i) { hipLaunchKernelGGL(k_touch, dim3(NBH), dim3(128), 0, s, a, (unsigned)i); });
        printf("depth %d + 8 b: %.1f MB per launch, (touch + attention) %.2f us, touch alone %.2f us -> attention %.2f us = %.2f TB/s (with the stamps)\n",
               base, bytes / 1e6, t, t0, t - t0, bytes / (t - t0) / 1e6);
        for (int rep = 0; rep < 3; ++rep) {
            hipLaunchKernelGGL(k_touch, dim3(NBH), dim3(128), 0, s, a, 77u + rep);
            hipLaunchKernelGGL((k_lm_attn_wave<128>), dim3(NBH, 1), dim3(256), 0, s, a);
            CK(hipStreamSynchronize(s));
            std::vector<long long> st((size_t)NBH * ATTN_NSTAMP);
            CK(hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_attn_stamps), st.size() * sizeof(long long)));
            long long first = st[0];
            for (int w = 0; w < NBH; ++w) first = std::min(first, st[(size_t)w * ATTN_NSTAMP]);
            printf("   run %d, us (100 MHz clock), min / median / max over %d workgroups:   since the workgroup's entry | since the launch's first entry\n", rep, NBH);
            for (int i = 0; i < 7; ++i) {
                std::vector<double> own(NBH), abs(NBH);
                for (int w = 0; w < NBH; ++w) {
                    own[w] = (st[(size_t)w * ATTN_NSTAMP + i] - st[(size_t)w * ATTN_NSTAMP]) * 0.01;
                    abs[w] = (st[(size_t)w * ATTN_NSTAMP + i] - first) * 0.01;
                }
                std::sort(own.begin(), own.end()); std::sort(abs.begin(), abs.end());
                printf("   %-20s %7.2f %7.2f %7.2f | %7.2f %7.2f %7.2f\n", stage[i], own[0], own[NBH / 2], own[NBH - 1], abs[0], abs[NBH / 2], abs[NBH - 1]);
            }
        }
    }
    uint16_t o4[4]; CK(hipMemcpy(o4, a.out, sizeof(o4), hipMemcpyDeviceToHost));
    printf("   first outputs of the last run (bf16 bits): %04x %04x %04x %04x\n", o4[0], o4[1], o4[2], o4[3]);
    return 0;
}
