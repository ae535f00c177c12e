// Every MMI_* environment variable the native library obeys, read in ONE place: mmi_knobs_from_env() is the only
// getenv in csrc/.  A handle (mmi_lm, mmi_mimi, mmi_duplex) takes one snapshot first thing in its create call and every later
// decision for it - create, streaming_start, program build, launch, the debug taps - reads handle->knobs: a variable changed
// after a handle exists does not reach that handle, only the handles created afterwards.  Unset = the shipped path.
#pragma once
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <string>
#include <vector>

struct MmiKnobs {
    static constexpr int UNSET = INT_MIN;       // "the variable is absent", where its presence alone or any integer means something

    // ---- both engines
    bool no_graph = false;          // MMI_NO_GRAPH=1 runs the same list eagerly, mirroring the reference's NO_CUDA_GRAPH switch ("0" = unset)
    char debug_poison = 0;          // MMI_DEBUG_POISON=1 (tests / scripts/gpu_check.sh): every allocation of a handle starts as 0xFF bytes
                                    // (bf16 / fp32 NaNs, int -1) instead of whatever the allocator hands out, so that a read of state the
                                    // engine never initialised shows up as a wrong result on every box; =0: zero-fill instead - two sessions
                                    // then start from identical memory, which is what MMI_DEBUG_TRACE's checksums need ('1' / '0' / 0 = unset)
    std::vector<std::string> skip_sites;   // MMI_SKIP_SITES="enc.tr,dec.res" (timing experiments ONLY - the outputs are then garbage): ops
                                    // whose site label starts with one of the prefixes are left out of the list

    // ---- LM engine: handle shape
    int lm_tile = 0;                // MMI_LM_TILE=32 / 16: A/B hook: the 32-row tile (and with it k_gemm_xlds / the octet sharing) at small batches
    int dep_tile = 0;               // MMI_DEP_TILE=16 (17..32 sessions, bf16): the depth transformer on two 16-row batch tiles (mmi_lm::Td)
    bool no_dep_in_group = false;   // MMI_NO_DEP_IN_GROUP=1: one depformer_in GEMM per micro-step instead of the grouped one
    // ---- LM engine: GEMM plans
    int gemm_ksplit = 0;            // MMI_GEMM_KSPLIT=1..4: test hook: force the split-K path on small shapes
    bool gemm_osplit_set = false;   // MMI_GEMM_OSPLIT present at all (even empty): k_gemm_q8 then shares no octets
    int gemm_osplit = UNSET;        // MMI_GEMM_OSPLIT: "0" = off, "2" / "4" = force (test hook / A-B), unset or empty = as many parts as bring
                                    // the launch to >= 128 workgroups
    bool gemm_osplit_all = false;   // "4a": every eligible GEMM (tests)
    char gemm_lds = 0;              // MMI_GEMM_LDS (its first character): "2" = k_gemm_xlds with the staggered tail, "1" = plain tails,
                                    // "0" = k_gemm_xp everywhere; 0 = unset: "2" for bf16 weights, "0" for int8 / fp8 ones (plan_xlds)
    int gemm_lds_grid = UNSET;      // MMI_GEMM_LDS_GRID: test hook: small grids / short chunks for the tiny shapes
    char gemm_once = 0;             // MMI_GEMM_ONCE=0: k_gemm_xp_once off (same-box A/B; bit-identical either way); "a": every bf16 GEMM whose
                                    // slices fit (test hook: the tiny shapes, always on 8 waves)
    bool no_norm_fusion = false;    // MMI_NO_NORM_FUSION=1: norm launch + GEMM instead of k_gemm_xp_norm / k_gemm_q8
    bool q8_act_bf16 = false;       // MMI_Q8_ACT=bf16: int8 linears weight-only (rounds 1-3) instead of int8 x int8
    bool q8_u2 = false;             // MMI_Q8_U=2: two entries per register buffer on int8 x int8 (the weight-only depth, same-box A/B)
    bool q8_tiles_serial = false;   // MMI_Q8_TILES=serial: k_gemm_q8 at 33..64 sessions walks both batch tiles in one workgroup (the round-4 form)
    // ---- LM engine: more than 64 model rows (mmi_lm_create_rows)
    bool rows_groups = false;       // MMI_ROWS_GROUPS=1: the A/B control of k_gemm_rows - the store / gate / RoPE GEMMs as one launch of the
                                    // <= 64-row kernels per group of two batch tiles (the weights cross HBM once per group)
    int rows_ntw = 0;               // MMI_ROWS_NTW=1 / 2: n-tiles per k_gemm_rows workgroup (same-box A/B; bit-identical); unset = by tile count
    // ---- LM engine: attention
    bool attn_split = false;        // MMI_ATTN: "wave" (default since round 4) = k_lm_attn_wave; "split" = the chunked kernel of rounds 1-3
    int attn_ns = 0;                // MMI_ATTN_NS=1..16: test hook: the split + combine path on rings too short to need it
    int attn_solo = UNSET;          // MMI_ATTN_SOLO=rows: test hook (0 = always the merge launch)
    bool attn_merge_kernel = false; // MMI_ATTN_MERGE=kernel (test hook) stays on variant 0 whatever the depth
    bool no_dep_attn_fusion = false;   // MMI_NO_DEP_ATTN_FUSION=1: the depth transformer's attention and out_proj as two launches
    bool dep_attn0_launch = false;  // MMI_DEP_ATTN0_LAUNCH=1 keeps the attention launch of micro-step 0
    bool no_precapture = false;     // MMI_NO_PRECAPTURE=1: the second attention step program is captured when first needed
    // ---- LM engine: debug
    bool debug_trace = false;       // MMI_DEBUG_TRACE=<prefix>: every step eagerly, every allocation checksummed after every op (mmi_lm::trace_file)
    std::string debug_trace_prefix;
    std::string debug_dump;         // MMI_DEBUG_DUMP="step:op:alloc[,alloc...]": those allocations, as they are after that op, to files

    // ---- Mimi engine
    int conv_mtb = 0;               // MMI_CONV_MTB=1|2|4, MMI_CONV_W=1|2|4|8: test hooks: the k_conv_wide tiling
    int conv_w = 0;
    int conv_ksplit = 0;            // MMI_CONV_KSPLIT=1..8: test hook: k_gemm_f32 split over workgroups
    long res_fusion_min = UNSET;    // MMI_MIMI_RES_FUSION_MIN: test hook: the tiny shapes on k_resblock
    bool mimi_no_align = false;     // MMI_MIMI_NO_ALIGN=1 keeps the dense layout of the audio-rate buffers (A/B)
    bool rvq_no_pair = false;       // MMI_RVQ_NO_PAIR=1: one RVQ level per launch pair
    bool mimi_pack_launches = false;   // MMI_MIMI_PACK_LAUNCHES=1: k_pack_b_f32 launches instead of producers writing the packed operand
    bool mimi_attn_two_pass = false;   // MMI_MIMI_ATTN_TWO_PASS=1: k_mimi_attn instead of k_mimi_attn_1pass
    bool mimi_two_commits = false;  // MMI_MIMI_TWO_COMMITS=1: k_commit_history + k_commit_counters instead of k_commit_all

    // ---- duplex pipeline
    int duplex_codec_cus = 0;       // MMI_DUPLEX_CODEC_CUS=n (experiment, round 6): the codec streams confined to n of the CUs (1..255)
    char duplex_prio = 0;           // MMI_DUPLEX_PRIO = codec / none select those stream priorities for an A/B ('c' / 'n')
};

// One line on stderr, once per process, for a variable that makes outputs invalid or moves work between streams
inline void mmi_knob_warn_once(std::atomic<bool>& said, const char* name, const char* value, const char* what) {
    if (!said.exchange(true)) fprintf(stderr, "moshi_mi: %s=%s is set: %s\n", name, value, what);
}

inline MmiKnobs mmi_knobs_from_env() {
    MmiKnobs k;
    auto present = [](const char* name) { return getenv(name) != nullptr; };
    auto first = [](const char* name) { const char* e = getenv(name); return e ? e[0] : (char)0; };
    auto number = [](const char* name, int absent) { const char* e = getenv(name); return e ? atoi(e) : absent; };
    auto one_of = [](int v, std::initializer_list<int> ok) { for (int o : ok) if (v == o) return v; return 0; };

    {
        const char* e = getenv("MMI_NO_GRAPH");
        k.no_graph = e && e[0] && e[0] != '0';
    }
    {
        const char p = first("MMI_DEBUG_POISON");
        k.debug_poison = p == '1' || p == '0' ? p : (char)0;
    }
    if (const char* e = getenv("MMI_SKIP_SITES")) {
        const std::string all(e);
        for (size_t i = 0; i <= all.size();) {
            const size_t j = all.find(',', i);
            const std::string pre = all.substr(i, j == std::string::npos ? std::string::npos : j - i);
            if (!pre.empty()) k.skip_sites.push_back(pre);
            if (j == std::string::npos) break;
            i = j + 1;
        }
        static std::atomic<bool> said{false};
        if (!k.skip_sites.empty()) mmi_knob_warn_once(said, "MMI_SKIP_SITES", e, "launch-list sites are left out, the outputs are garbage (timing experiments only)");
    }

    k.lm_tile = one_of(number("MMI_LM_TILE", 0), {16, 32});
    k.dep_tile = number("MMI_DEP_TILE", 0);
    k.no_dep_in_group = present("MMI_NO_DEP_IN_GROUP");
    {
        const int v = number("MMI_GEMM_KSPLIT", 0);
        k.gemm_ksplit = v >= 1 && v <= 4 ? v : 0;
    }
    if (const char* e = getenv("MMI_GEMM_OSPLIT")) {
        k.gemm_osplit_set = true;
        if (e[0]) { k.gemm_osplit = atoi(e); k.gemm_osplit_all = e[1] == 'a'; }
    }
    k.gemm_lds = first("MMI_GEMM_LDS");
    k.gemm_lds_grid = number("MMI_GEMM_LDS_GRID", MmiKnobs::UNSET);
    k.gemm_once = first("MMI_GEMM_ONCE");
    k.no_norm_fusion = present("MMI_NO_NORM_FUSION");
    k.q8_act_bf16 = first("MMI_Q8_ACT") == 'b';
    k.q8_u2 = first("MMI_Q8_U") == '2';
    k.q8_tiles_serial = first("MMI_Q8_TILES") == 's';
    {
        const char* e = getenv("MMI_ROWS_GROUPS");
        k.rows_groups = e && e[0] && e[0] != '0';
    }
    k.rows_ntw = one_of(number("MMI_ROWS_NTW", 0), {1, 2});
    k.attn_split = first("MMI_ATTN") == 's';
    {
        const int v = number("MMI_ATTN_NS", 0);
        k.attn_ns = v >= 1 && v <= 16 ? v : 0;
    }
    k.attn_solo = number("MMI_ATTN_SOLO", MmiKnobs::UNSET);
    k.attn_merge_kernel = first("MMI_ATTN_MERGE") == 'k';
    k.no_dep_attn_fusion = present("MMI_NO_DEP_ATTN_FUSION");
    k.dep_attn0_launch = present("MMI_DEP_ATTN0_LAUNCH");
    k.no_precapture = present("MMI_NO_PRECAPTURE");
    if (const char* e = getenv("MMI_DEBUG_TRACE")) { k.debug_trace = true; k.debug_trace_prefix = e; }
    if (const char* e = getenv("MMI_DEBUG_DUMP")) k.debug_dump = e;

    k.conv_mtb = one_of(number("MMI_CONV_MTB", 0), {1, 2, 4});
    k.conv_w = one_of(number("MMI_CONV_W", 0), {1, 2, 4, 8});
    {
        const int v = number("MMI_CONV_KSPLIT", 0);
        k.conv_ksplit = v >= 1 && v <= 8 ? v : 0;
    }
    if (const char* e = getenv("MMI_MIMI_RES_FUSION_MIN")) k.res_fusion_min = atol(e);
    k.mimi_no_align = present("MMI_MIMI_NO_ALIGN");
    k.rvq_no_pair = present("MMI_RVQ_NO_PAIR");
    k.mimi_pack_launches = present("MMI_MIMI_PACK_LAUNCHES");
    k.mimi_attn_two_pass = present("MMI_MIMI_ATTN_TWO_PASS");
    k.mimi_two_commits = present("MMI_MIMI_TWO_COMMITS");

    if (const char* e = getenv("MMI_DUPLEX_CODEC_CUS")) {
        const int v = atoi(e);
        static std::atomic<bool> said{false};
        if (v > 0 && v < 256) {
            k.duplex_codec_cus = v;
            mmi_knob_warn_once(said, "MMI_DUPLEX_CODEC_CUS", e, "the duplex pipeline's codec streams run on a CU mask (experiment)");
        } else if (e[0]) mmi_knob_warn_once(said, "MMI_DUPLEX_CODEC_CUS", e, "ignored, the CU count must be 1..255");
    }
    if (const char* e = getenv("MMI_DUPLEX_PRIO")) {
        static std::atomic<bool> said{false};
        if (e[0] == 'c' || e[0] == 'n') {
            k.duplex_prio = e[0];
            mmi_knob_warn_once(said, "MMI_DUPLEX_PRIO", e, "the duplex pipeline's stream priorities are not the shipped ones (A/B)");
        } else if (e[0]) mmi_knob_warn_once(said, "MMI_DUPLEX_PRIO", e, "ignored, the values are codec / none");
    }
    return k;
}
