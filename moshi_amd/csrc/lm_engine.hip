// Moshi LM engine behind the C ABI (include/moshi_mi.h): LMGen.step (reference: moshi/moshi/models/lm.py:668-850)
// = delay-ring bookkeeping + LMModel.forward_text (temporal transformer, lm.py:379-408) + text sampling +
// depformer_step (8 sequential depth-transformer micro-steps, lm.py:809-850, 450-493) as one fixed launch list over
// the kernels of lm_kernels.h, captured into a single hipGraph.
#include "lm_kernels.h"
#include "lm_prefill_kernels.h"
#include "lm_score_kernels.h"
#include "lm_logprob_kernels.h"
#include "mmi_fork_kernels.h"
#include "mmi_graph.h"

#include <math.h>
#include <stdio.h>
#include <map>

namespace {

struct GemmW {              // one packed nn.Linear
    u32x4* wp = nullptr;
    int N = 0, K = 0, NT = 0, KSTEPS = 0, gate = 0;   // gate: N = hidden, gate/value rows interleaved per tile
    float* scale = nullptr;   // int8 weights: SCB / 127 per original weight row; fp8: weight_scale * input_scale; KSTEPS then counts k-step PAIRS
    float* scb = nullptr;     // int8 weights: the raw SCB (`weight_scb`), for the int8 x int8 dequantisation (mmi_i8_dequant)
    int wq = 0;               // 0 bf16, 1 int8, 2 fp8, 4 MXFP4 (KSTEPS then counts entries of FOUR k-steps; scale / scb stay null)
    int ksteps = 0;           // MXFP4: the row's k-steps before padding to whole entries - what plan_gemm's thresholds count
    uint8_t* s4 = nullptr;    // MXFP4: the E8M0 scale bytes in entry order (k_pack_w_fp4)
    float xinv = 1.f;         // fp8: 1 / input_scale
    size_t bytes = 0;
    int T = 32;               // the MFMA tile the weight is packed for (lm->T; the depth transformer's linears: lm->Td) - also the
                              // tile of the packed activation operand it reads and of a packed output it writes
};

struct LayerW {
    GemmW in_proj, out_proj, ffn_in, ffn_out;
    uint16_t *n1 = nullptr, *n2 = nullptr;
    // cross-attention block (cfg.cross_attention; transformer.py:727-732): `cross_attention.in_projs.0` packed whole, with two
    // views of it - the query rows [0, dim) and the key / value rows [dim, 3 dim) - `out_projs.0`, and `norm_cross`
    GemmW x_in, x_q, x_kv, x_out;
    uint16_t *nx_w = nullptr, *nx_b = nullptr;
};

struct DepLayerW {
    std::vector<GemmW> in_proj, out_proj, ffn_in, ffn_out;   // per step
    uint16_t *n1 = nullptr, *n2 = nullptr;                   // shared by the steps
};

struct EvPair { hipEvent_t a, b; };

// The adapter bank of one linear (mmi_lm_enable_adapters): a = packed A_all [S * R][K] (a weight of S * R output rows at the
// linear's tile), b = packed bf16(scaling * B_all) [N][S * R] (a weight of S * R input features, gate / value rows interleaved
// like the linear's own); slot j owns rows / columns [j * R, (j + 1) * R), zero where nothing is loaded
struct LoraBank { u32x4* a = nullptr; u32x4* b = nullptr; };

// One buffer of a stream's device memory, declared ONCE: state_table() lists the streaming-state arena (mmi_lm::st), prefill_table()
// and score_table() the prefill arena.  The allocation, the start-up fill, mmi_lm_streaming_stop and mmi_lm_debug_state_regions all
// walk these lists.  The order of state_table() is the layout of a snapshot (mmi_lm_state_save): DESIGN.md section 2.
struct BufDecl {
    void** slot;                // the mmi_lm member that receives the pointer
    size_t elem, count;         // element size and count (an empty buffer still takes one element: MmiArena::alloc's rule)
    const char* name;
    int rows;                   // equal per-session slices, or 0
    int kind;                   // 1 = what a session is, 0 = rewritten before it is read (reported as `scratch<arena index>`)
    enum { UNTOUCHED, BYTES, I32 } init = UNTOUCHED;   // how it starts: as allocated, a byte fill, or ints through k_fill_i32
    int value = 0;
    size_t tail = 0;            // elements behind `count`, allocated and filled with it but outside the reported region
    int late = 0;               // the regions report lists the state buffers in table order, those with late > 0 behind them by
                                // ascending `late` (its line order is older than the table; tests/golden/lm_state_layout.json pins it)
    size_t off = 0, size = 0;   // where the arena holds it: set by alloc_table
    BufDecl& fill(int byte) { init = BYTES; value = byte; return *this; }
    BufDecl& fill_i32(int v) { init = I32; value = v; return *this; }
};

struct BufTable : std::vector<BufDecl> {
    template <class T>
    BufDecl& add(T** slot, size_t count, const char* name, int rows = 0, int kind = 0) {
        push_back(BufDecl{reinterpret_cast<void**>(slot), sizeof(T), count, name, rows, kind});
        return back();
    }
};

// The temporal ring of the stream (keys or values; filled at streaming_start).  bf16: an element each; e4m3: a byte each; 4-bit
// (MMI_F4E2M1X2): per layer the codes plane [B][H][cap][Dh/2] bytes, then the scale plane [B][H][cap][Dh/16] bytes.
struct KvRing {
    int form = 0;               // kv_form
    size_t elems = 0;           // values per layer: B * H * context * Dh
    size_t layer_u16 = 0;       // layer stride in uint16 units (kv_layer_u16: the 4-bit layer is padded)
    size_t codes_bytes = 0;     // bytes of a layer's values (the codes plane of the 4-bit form)
    size_t scale_off = 0;       // byte offset of the scale plane inside a 4-bit layer (elems / 16 bytes long), else 0
};

}  // namespace

struct mmi_lm {
    MmiKnobs knobs;                 // the MMI_* environment as it was when the handle was created (mmi_knobs.h)
    mmi_lm_cfg cfg;
    int device = -1;                // HIP device the handle lives on (current at create); see MmiDeviceGuard
    int max_batch = 0;
    int T = 32;                     // MFMA tile of the temporal transformer and the heads: 16 when max_batch <= 16, else 32 (lm_kernels.h)
    int Td = 32;                    // MFMA tile of the depth transformer (its linears, dx / dxn / datt / dhb): T.  knobs.dep_tile = 16 (17..32
                                    // sessions, bf16): two 16-row batch tiles per 16-row weight tile - measured in round 6 inside the step
                                    // (profiles/r06_logs/ab_dep_tile_once.txt): in_proj -0.14 us, linear_out -0.6, but the gated
                                    // linear_in +3.0 (352 tiles at 128 registers: spills) and out_proj +0.3 -> +0.15 ms per step; the
                                    // microbenchmark's -0.13 ms (round 5, independent launches) does not survive the dependent chain.
                                    // Kept as an opt-in: the boundaries are row-major either way (dpre, dqkv, the logits)
    int q8 = -1;                    // -1 undecided, 0 bf16 linears, 1 int8 linears (`weight` int8 + `weight_scb`, utils/quantize.py),
                                    // 2 fp8 linears (`weight` e4m3fn + `weight_scale` [+ `input_scale`]) run on the fp8 MFMA,
                                    // 4 MXFP4 linears (`weight` E2M1 pairs + `weight_scale_e8m0`), widened to bf16 in the GEMM
    int NC = 0, CT = 0, max_delay = 0;
    MmiArena wts;
    // weights
    uint16_t* emb = nullptr;        // [n_q][card+1][dim]
    uint16_t* text_emb = nullptr;   // [text_card+1][dim]
    std::vector<LayerW> layers;
    uint16_t* out_norm = nullptr;
    GemmW text_linear;
    std::vector<GemmW> dep_in, dep_lin;
    GemmW dep_in_all;               // the dep_q depformer_in linears as one [dep_q * depformer_dim, dim] GEMM
    bool dep_in_grouped = false;
    std::vector<uint16_t*> dep_emb; // [0] = depformer_text_emb, [k>=1] = depformer_emb[k-1] (low-rank ones expanded at create)
    // mmi_lm_cfg_ext (TTS family): micro-step k runs depformer weight set dep_sched[k] of dep_nw (identity without a schedule);
    // a demuxed text stream embeds through text_emb | text_emb2 (out1 / out2 of text_emb) and dep_emb[0] | dep_emb2
    std::vector<int> dep_sched;
    int dep_nw = 0;
    bool demux = false;
    bool dep_low_rank = false;      // depformer_low_rank_embeddings (the tables are expanded at create)
    uint16_t *text_emb2 = nullptr, *dep_emb2 = nullptr;
    std::vector<DepLayerW> dep_layers;
    // parity tap (mmi_lm_debug_linear): every packed linear / every norm vector by its state-dict key
    std::map<std::string, GemmW> linear_by_name;
    std::map<std::string, const uint16_t*> vector_by_name;
    int* delays_dev = nullptr;
    size_t weight_bytes = 0;
    // streaming state
    bool streaming = false;
    int batch = 0;                  // MODEL rows: the sessions, doubled under classifier-free guidance (lm.py:646-651)
    int gen_batch = 0;              // sessions (rows of the token ring, the samplers and the caller's tensors)
    float cfg_coef = 1.f;           // LMGen(cfg_coef, cfg_is_no_text, cfg_is_masked_until) (lm.py:566-574)
    int cfg_no_text = 0;
    int* masked_until = nullptr;    // [gen_batch] or null
    uint16_t* cond = nullptr;       // [batch][dim] summed `sum` conditions (lm.py:621-628) or null
    uint16_t* xkv = nullptr;        // [layers][batch][cross_cap][2 * dim] keys | values of every model row's cross-attention source
    int cross_len = 0;              // mmi_guidance.cross_len of the stream's start
    int cross_cap = 0;              // positions a row's source may hold for this stream (cross_cap_set, or cross_len)
    int cross_cap_set = 0;          // mmi_lm_set_cross_capacity; 0 = the start's cross_len
    int* xlen = nullptr;            // [batch] live positions per model row (k_lm_cross_attn), null without cross-attention
    float* coefs = nullptr;         // [gen_batch] guidance coefficient per session (k_cfg_mix)
    long* offsets_m = nullptr;      // [batch] offsets per model row (== offsets without guidance)
    std::vector<uint16_t*> extra_heads;   // nn.Linear(dim, extra_heads_dim) weights, row-major
    uint16_t* extra_heads_all = nullptr;
    mmi_sampling samp;
    int kmax = 0;
    MmiArena st;
    BufTable st_table;              // what `st` holds, in allocation order (state_table): entry i is allocation i of the arena
    KvRing ring;
    uint8_t* exec = nullptr;
    long* offsets = nullptr;
    int* cache = nullptr;
    int* user_i32 = nullptr;
    int* tokens = nullptr;          // [B][NC] model input
    int* text_tok = nullptr;        // [B]
    int* audio_tok = nullptr;       // [B][dep_q]
    int* out_i32 = nullptr;         // [B][dep_q+1]
    uint16_t *x = nullptr, *xn = nullptr, *qrot = nullptr, *att = nullptr, *hb = nullptr;
    uint16_t *tout = nullptr, *text_logits = nullptr;
    uint16_t *kc = nullptr, *vc = nullptr;          // [layers][B][H][cap][Dh]
    float *opart = nullptr, *ml = nullptr;
    unsigned* attn_done = nullptr;                  // [B][H] arrival counters of the split decode attention (k_lm_attn_wave), 0 between launches
    float* partial = nullptr;                       // [4][B][max(dim, depformer_dim)] split-K partial sums
    float* rope = nullptr;                          // [B][Dh/2][2] (cos, sin) of the step's new position
    // int8 activations (BASELINE configs[4], the reference's own arithmetic: QLinear.forward -> bitsandbytes' int8 x int8 matmul,
    // utils/quantize.py:24-40): on for int8 linears unless knobs.q8_act_bf16 (weight-only, rounds 1-3) or the model has
    // cross-attention layers.  xnq / attq / hbq / toutq: the int8 operand Xq[mt][kp][lane][16] next to its bf16 tensor, sx_*: its
    // rows' absmax (bitsandbytes' SCA).  Who quantises: the norm kernel for its own output (one workgroup per row); a
    // k_quant_rows_i8 launch for the temporal attention output and the gated FFN tensor (rows written by many workgroups); the
    // depth transformer's GEMMs themselves (k_gemm_q8: every workgroup holds the whole short row).  No atomics: absmax slots
    // folded by the producing epilogues were built first and measured - 704 gated tiles x 64 rows hammering 2 cache lines took
    // linear_in from 50 to 94 us (58 with test-then-max), profiles/r04_logs/call_b_summary.txt.
    bool act8 = false;
    uint8_t *xnq = nullptr, *attq = nullptr, *hbq = nullptr, *toutq = nullptr, *dxnq = nullptr;
    float *sx_xn = nullptr, *sx_tout = nullptr, *sx_dxn = nullptr, *sx_att = nullptr, *sx_hb = nullptr;
    bool hidden_taps = false;                       // mmi_lm_set_hidden_taps: the next streaming_start adds the two copies below
    uint16_t* htap = nullptr;                       // [2][B][dim] residual stream after the first / the last temporal layer
    uint16_t *dx = nullptr, *dxn = nullptr, *dqkv = nullptr, *datt = nullptr, *dhb = nullptr, *dlogits = nullptr;
    uint16_t* dpre = nullptr;       // [B][dep_q * depformer_dim] depformer_in[k](transformer_out) of every micro-step
    uint16_t *dkc = nullptr, *dvc = nullptr;        // [dep_layers][B][Hd][dep_q][Dhd]
    float* noise = nullptr;                         // [B][1+dep_q][kmax]
    int* use_noise = nullptr;
    int* forced = nullptr;                          // [B][1+dep_q]
    int* use_forced = nullptr;
    bool forced_armed = false;
    bool noise_on = false;                          // host mirror of *use_noise
    unsigned long long* rng = nullptr;
    // per-session sampling (mmi_lm_set_row_sampling): the device table k_sample reads, the rings of committed text tokens, and
    // the host's mirror of `active` (supplied noise is refused while any row is active)
    RowSamp* rowtab = nullptr;                      // [gen_batch]
    int* thist = nullptr;                           // [gen_batch][MMI_TEXT_HIST]
    std::vector<uint8_t> row_active;
    // nucleus sampling (mmi_lm_enable_nucleus): the handle's values, whether this stream runs k_sample_nucleus, and
    // the host's mirror of the sessions' effective values behind rowtab (supplied noise is refused while any is positive)
    bool nucleus_on = false, nucleus_live = false;
    float top_p = 0.f, top_p_text = 0.f;
    std::vector<RowTopP> row_top_p;
    int text_eop = 0;                              // LMModel.end_of_text_padding_id (mmi_lm_set_text_end_padding_id)
    // per-step host hooks (mmi_lm_set_hooks): the step is cut at these ops of the launch list
    mmi_lm_hooks hooks{nullptr, nullptr, nullptr, nullptr};
    bool in_hook = false;
    size_t op_text_sample = 0, op_after_text_sample = 0, op_commit = 0;
    size_t op_depformer = 0;        // first op after the temporal transformer + text head: where mmi_lm_set_phase_event's event is recorded
    int (*phase_fn)(void*, mmi_stream) = nullptr;   // mmi_lm_set_phase_callback
    void* phase_user = nullptr;
    SampleArgs text_sample_args;    // to rebuild the depth transformer's first input when a hook changed the text token
    // the TTS script machine (mmi_lm_enable_tts_machine): parameters and capacities belong to the handle, the rows to the stream
    bool tts_on = false;
    TtsParams tts_p{};
    int tts_max_entries = 0, tts_max_tokens = 0, tts_max_prefix = 0;
    int tts_stride = 0;             // ints per session row (lm_kernels.h: header + arrays)
    int* tts = nullptr;             // [gen_batch][tts_stride], streaming-state arena
    int* tts_stage = nullptr;       // pinned [gen_batch][tts_stride]: mmi_lm_set_row_script composes a row here and copies it
    std::vector<hipEvent_t> tts_stage_ev;     // behind the copy out of a session's staging row; waited for before it is reused
    std::vector<uint8_t> tts_stage_used;
    bool tts_rule_done = false;     // this (hooked) step has applied the audio rule in front of on_audio_tokens: the commit does not
    // per-row LoRA adapters, unmerged (modules/lora.py): the banks belong to the handle, the slot table to the stream
    bool lora_on = false;
    int lora_S = 0, lora_R = 0;     // max_adapters, max_rank
    MmiArena lora_mem;
    std::map<const void*, LoraBank> lora_by_wp;       // by the packed weight (GemmW::wp) of the linear
    std::map<std::string, const void*> lora_by_name;  // `<linear>.weight` -> that key
    int* lora_bad = nullptr;        // device flag of mmi_lm_load_adapter's finiteness check
    int* row_slot = nullptr;        // [gen_batch] adapter slot per session, -1 = none (streaming-state arena: snapshots carry it)
    std::vector<int> row_slot_h;    // the host's mirror (a slot is not reloaded while a live row selects it)
    uint16_t* lora_t = nullptr;     // packed t = bf16(A x) of the linear in flight (adapters need Td == T: one tile, one buffer)
    // chunked prefill (mmi_lm_enable_prefill): the row budget of a pass belongs to the handle, the scratch of a pass
    // to the stream - an arena of its own, so that the streaming-state arena (mmi_lm_state_bytes, snapshots) is what it was
    int prefill_rows = 0;
    MmiArena pf_mem;
    BufTable pf_table;              // what `pf_mem` holds (prefill_table, then score_table)
    struct {
        int* tokens = nullptr;          // [rows][NC] model input
        int* row_sess = nullptr;        // [rows]
        long* row_pos = nullptr;        // [rows]
        float* rope = nullptr;          // [rows][Dh/2][2]
        uint16_t *x = nullptr, *xn = nullptr, *att = nullptr, *hb = nullptr;      // packed activations of `rows` rows
        uint16_t *qkv = nullptr, *q = nullptr;                                    // row-major in_proj output, roped queries
        uint8_t *sk = nullptr, *sv = nullptr, *sks = nullptr, *svs = nullptr;     // the staged block in ring format
        float* partial = nullptr;       // [4][rows][dim] split-K partial sums
    } pf;
    // teacher-forced scoring on the prefill path (mmi_lm_enable_score): scratch of its own in the prefill arena - the
    // step's depth-transformer cache (dkc / dvc) and activations are not touched, so a score call between two steps changes nothing
    // a neighbour reads
    bool score_on = false;
    struct {
        uint16_t* tout = nullptr;       // packed transformer_out of the pass's rows
        uint16_t* tlog = nullptr;       // [rows][text_card_out] bf16 text logits
        int* targets = nullptr;         // [rows][1 + dep_q] the given tokens of the pass
        uint16_t* dpre = nullptr;       // [rows][depformer_dim] depformer_in of the micro-step in flight
        uint16_t *dx = nullptr, *dxn = nullptr, *datt = nullptr, *dhb = nullptr;   // packed at the depth transformer's tile
        uint16_t* dqkv = nullptr;       // [rows][3 * depformer_dim]
        uint16_t *dkc = nullptr, *dvc = nullptr;        // [dep_layers][rows][Hd][dep_q][Dhd]
        uint16_t* alog = nullptr;       // [dep_q][rows][card] bf16 audio logits
    } sc;
    // log-probabilities in the live step (mmi_lm_enable_logprobs): the option belongs to the handle, the float rings
    // to the stream - an arena of its own beside the streaming-state arena, so that mmi_lm_state_bytes and snapshots are what they were
    bool lp_on = false;
    int lp_top_n = 0;
    MmiArena lp_mem;
    LpRings lp{nullptr, nullptr, nullptr, 0, 0};    // lp.lp != null: this stream records them
    long offset_cpu = 0;
    int attn_ns = 1;                                // workgroups per (session, head) of the decode attention (attn_splits)
    long depth_bound = 0;                           // no session's offset exceeds this (steps since streaming_start / the last seek; resets
                                                    // only lower offsets): picks the step program's variant (attn_variant)
    long xlds_launches = 0;         // launches (or graph nodes captured) that took k_gemm_xlds: mmi_lm_stat(lm, 0)
    long rows_launches = 0;         // launches (or graph nodes captured) that took k_gemm_rows: mmi_lm_stat(lm, 4)
                                    // (both count every launch_gemm: the GEMMs of a prefill pass as well as a step's)
    bool precapture_failed = false; // capturing the second attention program ahead of time failed once: not tried again for this stream
    bool dominant_xlds = false;     // the profiled (dominant) GEMM ran on k_gemm_xlds
    MmiProgram prog;
    // knobs.debug_trace (debug: finding which launch of the step is not reproducible): every step runs its launch list
    // eagerly and, after EVERY op, checksums every allocation of the streaming state; lines "step op site allocation bytes
    // checksum" for the allocations an op changed go to <prefix>.<n> (n = streaming sessions of the process so far).  Two
    // sessions fed the same inputs must write the same file.
    FILE* trace_file = nullptr;
    std::string trace_name;
    unsigned long long* trace_dev = nullptr;
    std::vector<unsigned long long> trace_prev;
    long trace_step = 0;
    hipStream_t cap_stream = nullptr;
    bool use_graph = true;
    // profiling tap
    struct SiteEv { size_t op; hipEvent_t ev; };
    std::vector<SiteEv> site_ev;     // one event in front of every eagerly run op while profiling, one behind the step's last
                                     // (op = SIZE_MAX): an op's time is the distance to the next event (mmi_lm_profile_sites)
    size_t site_ev_used = 0;
    bool profiling = false;
    std::vector<EvPair> ev_pool;
    size_t ev_used = 0;
    hipStream_t prof_stream = nullptr;
    long prof_bytes = 0;
};

namespace {

int need(const MmiWeights& W, const std::string& name, int ndim, const mmi_tensor_desc** out) {
    const mmi_tensor_desc* d = W.find(name);
    if (!d) return mmi_fail(MMI_ERR_MISSING_WEIGHT, "missing weight: " + name);
    if (d->dtype != MMI_BF16) return mmi_fail(MMI_ERR_UNSUPPORTED, "LM weights must be bf16: " + name);
    if (d->ndim != ndim) return mmi_fail(MMI_ERR_SHAPE, "unexpected rank for " + name);
    *out = d;
    return MMI_OK;
}

// nn.Linear weight [N][K] -> packed; gate_hidden > 0: [2*hidden][K] gate|value matrix
__global__ void k_scb_to_scale(const float* __restrict__ scb, float* __restrict__ scale, int n, float mul, float div) {
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) scale[i] = scb[i] * mul / div;
}

// wp_dst / scale_dst: pack into a slice of a caller-owned allocation instead of a fresh one (see load_dep_in_group)
int load_linear(mmi_lm* lm, const MmiWeights& W, const std::string& name, int N, int K, int gate_hidden, GemmW* g,
                void* wp_dst = nullptr, float* scale_dst = nullptr, float* scb_dst = nullptr, int tile = 0, uint8_t* s4_dst = nullptr) {
    const mmi_tensor_desc* d = W.find(name);
    if (!d) return mmi_fail(MMI_ERR_MISSING_WEIGHT, "missing weight: " + name);
    if (d->dtype != MMI_BF16 && d->dtype != MMI_I8 && d->dtype != MMI_F8E4M3 && d->dtype != MMI_F4E2M1X2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "LM linear weights must be bf16, int8 or fp8 (e4m3fn): " + name);
    if (d->ndim != 2) return mmi_fail(MMI_ERR_SHAPE, "unexpected rank for " + name);
    const int q8 = d->dtype == MMI_I8 ? 1 : (d->dtype == MMI_F8E4M3 ? 2 : (d->dtype == MMI_F4E2M1X2 ? 4 : 0));
    if (lm->q8 >= 0 && lm->q8 != q8) return mmi_fail(MMI_ERR_UNSUPPORTED, "mixed bf16 / int8 / fp8 linear weights: " + name);
    lm->q8 = q8;
    if (q8 == 4 && K % 32 != 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "MXFP4 linears need in_features to be a multiple of 32: " + name);
    if (d->shape[0] != N || d->shape[1] != (q8 == 4 ? K / 2 : K)) return mmi_fail(MMI_ERR_SHAPE, "shape mismatch for " + name);
    if (K % 8 != 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "in_features must be a multiple of 8: " + name);
    const int TN = tile ? tile : lm->T;
    g->T = TN;
    g->K = K;
    g->gate = gate_hidden > 0 ? 1 : 0;
    g->N = gate_hidden > 0 ? gate_hidden : N;
    if (g->N % 8 != 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "out_features must be a multiple of 8: " + name);
    const int rows_per_tile = gate_hidden > 0 ? TN / 2 : TN;
    g->NT = mmi_cdiv(g->N, rows_per_tile);
    const int ksteps = mmi_cdiv(K, mmi_kstep(TN));
    if (q8 == 4) {
        // `<linear>.weight_scale_e8m0`: one byte per 32 input features of a row (its values were checked by check_mxfp4_descs)
        const std::string sname = name + "_scale_e8m0";
        const mmi_tensor_desc* sc = W.find(sname);
        if (!sc) return mmi_fail(MMI_ERR_MISSING_WEIGHT, "missing weight: " + sname);
        if (sc->dtype != MMI_E8M0 || sc->ndim != 2 || sc->shape[0] != N || sc->shape[1] != K / 32)
            return mmi_fail(MMI_ERR_SHAPE, "MXFP4 block scales must be e8m0 [out_features, in_features / 32]: " + sname);
        g->wq = 4;
        g->KSTEPS = mmi_cdiv(ksteps, 4);                       // entries of four k-steps
        g->ksteps = ksteps;
        const size_t n = (size_t)g->NT * g->KSTEPS * 1024, ns = (size_t)g->NT * g->KSTEPS * 64 * (TN == 32 ? 2 : 4);
        uint8_t* p = reinterpret_cast<uint8_t*>(wp_dst);
        if (!p) MMI_HIP_CHECK(lm->wts.alloc(&p, n));
        g->wp = reinterpret_cast<u32x4*>(p);
        g->s4 = s4_dst;
        if (!g->s4) MMI_HIP_CHECK(lm->wts.alloc(&g->s4, ns));
        g->bytes = n + ns;                                     // 0.5 B per weight + the scale bytes as the GEMM streams them
        MMI_LAUNCH(k_pack_w_fp4, (int)mmi_cdiv64((int64_t)n, 256), 256, 0, (hipStream_t)0, (const uint8_t*)d->data, (const uint8_t*)sc->data,
                   p, g->s4, N, K, TN, g->NT, g->KSTEPS, gate_hidden);
    } else if (!q8) {
        g->KSTEPS = ksteps;
        size_t n = (size_t)g->NT * g->KSTEPS * 512;
        uint16_t* p = reinterpret_cast<uint16_t*>(wp_dst);
        if (!p) MMI_HIP_CHECK(lm->wts.alloc(&p, n));
        g->wp = reinterpret_cast<u32x4*>(p);
        g->bytes = n * sizeof(uint16_t);
        MMI_LAUNCH(k_pack_w_bf16, (int)mmi_cdiv64((int64_t)n, 256), 256, 0, (hipStream_t)0, (const uint16_t*)d->data, p, N, K,
                   TN, g->NT, g->KSTEPS, gate_hidden);
    } else {
        // int8: `<linear>.weight_scb` = row absmax (utils/quantize.py:20-22).  fp8: `<linear>.weight_scale` = dequantisation
        // factor per row, and an optional scalar `<linear>.input_scale` (static activation scale, default 1)
        const std::string stem = name.size() > 7 && name.compare(name.size() - 7, 7, ".weight") == 0 ? name.substr(0, name.size() - 7) : name;
        const std::string sname = q8 == 1 ? name + "_scb" : name + "_scale";
        const mmi_tensor_desc* sc = W.find(sname);
        if (!sc) return mmi_fail(MMI_ERR_MISSING_WEIGHT, "missing weight: " + sname);
        if (sc->dtype != MMI_F32 || sc->shape[0] != N) return mmi_fail(MMI_ERR_SHAPE, "row scales must be fp32 [out_features]: " + sname);
        float in_scale = 1.f;
        if (q8 == 2) {
            if (const mmi_tensor_desc* is = W.find(stem + ".input_scale")) {
                if (is->dtype != MMI_F32) return mmi_fail(MMI_ERR_SHAPE, "input_scale must be fp32: " + stem);
                MMI_HIP_CHECK(hipMemcpy(&in_scale, is->data, sizeof(float), hipMemcpyDeviceToHost));
                if (!(in_scale > 0.f)) return mmi_fail(MMI_ERR_INVALID, "input_scale must be positive: " + stem);
            }
        }
        g->wq = q8;
        g->xinv = 1.f / in_scale;
        g->KSTEPS = mmi_cdiv(ksteps, 2);                       // pairs of k-steps
        size_t n = (size_t)g->NT * g->KSTEPS * 1024;
        int8_t* p = reinterpret_cast<int8_t*>(wp_dst);
        if (!p) MMI_HIP_CHECK(lm->wts.alloc(&p, n));
        g->wp = reinterpret_cast<u32x4*>(p);
        g->scale = scale_dst;
        if (!g->scale) MMI_HIP_CHECK(lm->wts.alloc(&g->scale, (size_t)N));
        if (q8 == 1) {
            g->scb = scb_dst;
            if (!g->scb) MMI_HIP_CHECK(lm->wts.alloc(&g->scb, (size_t)N));
            MMI_HIP_CHECK(hipMemcpy(g->scb, sc->data, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice));
        }
        g->bytes = n + (size_t)N * sizeof(float);
        MMI_LAUNCH(k_pack_w_i8, (int)mmi_cdiv64((int64_t)n, 256), 256, 0, (hipStream_t)0, (const int8_t*)d->data, p, N, K, TN,
                   g->NT, g->KSTEPS, gate_hidden);
        MMI_LAUNCH(k_scb_to_scale, mmi_cdiv(N, 256), 256, 0, (hipStream_t)0, (const float*)sc->data, g->scale, N,
                   q8 == 1 ? 1.f : in_scale, q8 == 1 ? 127.f : 1.f);
    }
    lm->weight_bytes += g->bytes;
    lm->linear_by_name[name] = *g;
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

int load_copy(mmi_lm* lm, const MmiWeights& W, const std::string& name, int ndim, size_t n, uint16_t** out, uint16_t* into = nullptr) {
    const mmi_tensor_desc* d;
    int rc = need(W, name, ndim, &d);
    if (rc) return rc;
    size_t have = 1;
    for (int i = 0; i < d->ndim; ++i) have *= (size_t)d->shape[i];
    if (have != n) return mmi_fail(MMI_ERR_SHAPE, "shape mismatch for " + name);
    uint16_t* dst = into;
    if (!dst) MMI_HIP_CHECK(lm->wts.alloc(&dst, n));
    MMI_HIP_CHECK(hipMemcpy(dst, d->data, n * sizeof(uint16_t), hipMemcpyDeviceToDevice));
    if (out) *out = dst;
    lm->vector_by_name[name] = dst;
    return MMI_OK;
}

// `<stem>.weight` [V][R] through the nn.Linear(R, D) `<stem><suffix>` [D][R], expanded once into a full [V][D] bf16 table
// (k_expand_emb): what a low-rank or demuxed embedding (lm_utils.py:95-124) computes for every token, gathered per step
int load_expanded(mmi_lm* lm, const MmiWeights& W, const std::string& stem, int V, int R, int D, const char* suffix, uint16_t** out) {
    const mmi_tensor_desc *e, *w;
    int rc = need(W, stem + ".weight", 2, &e);
    if (rc || (rc = need(W, stem + suffix, 2, &w))) return rc;
    if (e->shape[0] != V || e->shape[1] != R) return mmi_fail(MMI_ERR_SHAPE, "shape mismatch for " + stem + ".weight");
    if (w->shape[0] != D || w->shape[1] != R) return mmi_fail(MMI_ERR_SHAPE, "shape mismatch for " + stem + suffix);
    uint16_t* dst = nullptr;
    MMI_HIP_CHECK(lm->wts.alloc(&dst, (size_t)V * D));
    MMI_LAUNCH(k_expand_emb, dim3(mmi_cdiv(D, 256), V), 256, 0, (hipStream_t)0, (const uint16_t*)e->data, R, (const uint16_t*)w->data, D, dst);
    MMI_CHECK_LAUNCH();
    *out = dst;
    lm->vector_by_name[stem + suffix] = dst;
    return MMI_OK;
}

// ---- launch helpers ---------------------------------------------------------------------------
struct GemmPlan { int waves, ntw, ksplit, u, osplit; };

// How a GEMM is cut into workgroups (measured on MI355X with scripts/gemm_microbench.hip): enough workgroups to
// cover the 256 CUs, K split over the waves of a workgroup, more waves per workgroup when there are few n-tiles.
GemmPlan plan_gemm(const MmiKnobs& k, const GemmW& g, bool may_split) {
    GemmPlan p;
    p.ntw = 1;
    p.ksplit = 1;
    // few n-tiles (N = 4096 at the 32-row tile): split K over workgroups so that every CU streams weights
    // (the thresholds count k-steps: an MXFP4 linear, whose KSTEPS are entries of four, is planned from the k-steps of its row -
    // the split-K and wave plan of its bf16 twin, also where the row is no whole number of entries)
    const int kst = g.wq == 4 ? g.ksteps : g.KSTEPS;
    if (may_split && g.NT < 200 && kst >= 128) p.ksplit = g.NT <= 64 ? 4 : 2;
    if (k.gemm_ksplit && may_split && g.KSTEPS >= k.gemm_ksplit) p.ksplit = k.gemm_ksplit;      // test hook: force the split-K path
    const int ks = kst / p.ksplit;
    p.waves = ks >= 32 ? 8 : 4;
    // fragments in flight per register buffer: 2 for the widest GEMM (the temporal FFN linear_in, 704 n-tiles: fewer
    // registers -> 3 workgroups per CU -> all 704 resident at once; 36.8 vs 39.3 us in the microbenchmark), else 4
    p.u = (g.gate && g.NT >= 512 && p.waves == 8) ? 2 : 4;
    if (g.scale) p.u = 2;            // int8 entries carry two k-steps each
    // (two n-tiles per workgroup for the 384-tile temporal in_proj look 3.5 us faster in the microbenchmark - 22.5 against
    // 26.0 us, profiles/r01_logs/gemm_microbench_b32_v10.txt - and make no difference in the step: 8.176 / 8.186 ms against
    // 8.190 / 8.176 ms in a same-box A/B, profiles/r01_logs/ab_in_proj_ntw2.txt; not adopted)
    p.osplit = 1;
    return p;
}

// Octet sharing of k_gemm_xp (GemmArgs::osplit): GEMMs with so few n-tiles that most CUs would idle while each busy one is
// bound by what a single CU can pull (~25 GB/s) - the depth transformer's N = 1024 linears: 32 tiles of 64-180 KB.
// knobs.gemm_osplit: 0 = off, 2 / 4 = force (test hook / A-B), default = as many parts as bring the launch to >= 128 workgroups.
// pairs: the in_proj of a 4-bit ring - a part must own whole octet PAIRS (a ring block is 16 features: mmi_epi_kv_feats), so
// two parts at the 32-row tile at most, none at the 16-row tile.
int plan_osplit(const MmiKnobs& k, const GemmW& g, const GemmPlan& p, int epi, int T, bool pairs = false) {
    if (epi == MMI_EPI_GATE || g.wq != 0 || p.ntw != 1 || (T != 32 && T != 16)) return 1;
    const int octs = pairs ? T / 16 : T / 8;
    int os = 1;
    if (k.gemm_osplit != MmiKnobs::UNSET) {
        if (k.gemm_osplit <= 1) return 1;
        os = k.gemm_osplit < octs ? k.gemm_osplit : octs;
        if (k.gemm_osplit_all) return os;      // "4a": every eligible GEMM (tests)
        return (long)g.NT * p.ksplit <= 64 ? os : 1;
    }
    while (os < octs && (long)g.NT * p.ksplit * os < 128) os *= 2;
    return (long)g.NT * p.ksplit <= 64 ? os : 1;
}

template <int TN, int MT, int NTW, int WQ, bool KV4 = false>
int launch_gemm_q(hipStream_t s, dim3 groups, int waves, const GemmArgs& a) {
    if constexpr (MT * NTW <= 2) {
        if (waves == 8) MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 8, 2, WQ, false, false, KV4>), groups, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 4, 2, WQ, false, false, KV4>), groups, 256, 0, s, a);
    } else {
        MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 4, 2, WQ, false, false, KV4>), groups, 256, 0, s, a);
    }
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// MXFP4 entries (four k-steps each): two entries per register buffer at one batch tile, one at two (8 activation fragments per
// entry there); no instantiation carries scratch (profiles/mxfp4/kernel_resources.csv)
template <int TN, int MT, int NTW, bool KV4 = false>
int launch_gemm_f4(hipStream_t s, dim3 groups, int waves, const GemmArgs& a) {
    constexpr int U = MT == 1 ? 2 : 1;
    if constexpr (MT * NTW <= 2) {
        if (waves == 8) MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 8, U, 4, false, false, KV4>), groups, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 4, U, 4, false, false, KV4>), groups, 256, 0, s, a);
        MMI_CHECK_LAUNCH();
        return MMI_OK;
    }
    return mmi_fail(MMI_ERR_UNSUPPORTED, "MXFP4 linears run one n-tile and at most two batch tiles per workgroup");
}

template <int TN, int MT, int NTW, bool KV4 = false>
int launch_gemm_w(hipStream_t s, dim3 groups, int waves, int u, int wq, bool q8_u2, const GemmArgs& a) {
    if (wq == 4) return launch_gemm_f4<TN, MT, NTW, KV4>(s, groups, waves, a);
    if (wq == 1) return launch_gemm_q<TN, MT, NTW, 1, KV4>(s, groups, waves, a);
    if (wq == 2) return launch_gemm_q<TN, MT, NTW, 2, KV4>(s, groups, waves, a);
    if (wq == 3) {
        // int8 x int8 has no conversion to hold in registers: four entries per register buffer instead of two (q8_u2: the
        // weight-only depth, same-box A/B)
        if (!q8_u2 && waves == 8) {
            if constexpr (MT * NTW <= 2) {
                MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 8, 4, 3, false, false, KV4>), groups, 512, 0, s, a);
                MMI_CHECK_LAUNCH();
                return MMI_OK;
            }
        }
        return launch_gemm_q<TN, MT, NTW, 3, KV4>(s, groups, waves, a);
    }
    if (waves == 8 && u == 2 && MT * NTW == 1) {
        if constexpr (MT * NTW == 1) MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 8, 2, 0, false, false, KV4>), groups, 512, 0, s, a);
        MMI_CHECK_LAUNCH();
        return MMI_OK;
    }
    switch (waves) {
        case 4: MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 4, 4, 0, false, false, KV4>), groups, 256, 0, s, a); break;
        case 8:
            if constexpr (MT * NTW <= 2) { MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 8, 4, 0, false, false, KV4>), groups, 512, 0, s, a); break; }
            MMI_LAUNCH((k_gemm_xp<TN, MT, NTW, 4, 4, 0, false, false, KV4>), groups, 256, 0, s, a); break;
        default: return mmi_fail(MMI_ERR_UNSUPPORTED, "unsupported waves per GEMM workgroup");
    }
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

template <int TN, bool KV4 = false>
int launch_gemm_t(hipStream_t s, const GemmPlan& p, int NT, int mt, bool q8_u2, const GemmArgs& a) {
    const dim3 groups(mmi_cdiv(NT, p.ntw) * (a.osplit > 1 ? a.osplit : 1), p.ksplit);
    const int w8 = a.wq;
    if (mt == 1) return launch_gemm_w<TN, 1, 1, KV4>(s, groups, p.waves, p.u, w8, q8_u2, a);     // one n-tile per workgroup (two measured slower
    if (mt == 2) return launch_gemm_w<TN, 2, 1, KV4>(s, groups, p.waves, p.u, w8, q8_u2, a);     // in the step, DESIGN 9e: not instantiated)
    return mmi_fail(MMI_ERR_UNSUPPORTED, "batch too large for the skinny GEMM");
}

// Adapter handles (mmi_lm_enable_adapters): the LORA forms of k_gemm_xp - bf16, one n-tile per workgroup, at most two batch
// tiles - under launch_gemm_w's choice of waves and fragments in flight
template <int TN, int MT, bool KV4 = false>
int launch_gemm_lora(hipStream_t s, dim3 groups, int waves, int u, const GemmArgs& a) {
    if (waves == 8 && u == 2 && MT == 1) {
        if constexpr (MT == 1) MMI_LAUNCH((k_gemm_xp<TN, MT, 1, 8, 2, 0, true, false, KV4>), groups, 512, 0, s, a);
    } else if (waves == 8) MMI_LAUNCH((k_gemm_xp<TN, MT, 1, 8, 4, 0, true, false, KV4>), groups, 512, 0, s, a);
    else if (waves == 4) MMI_LAUNCH((k_gemm_xp<TN, MT, 1, 4, 4, 0, true, false, KV4>), groups, 256, 0, s, a);
    else return mmi_fail(MMI_ERR_UNSUPPORTED, "unsupported waves per GEMM workgroup");
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}
template <int TN, int MT>
int launch_lora_shrink_t(hipStream_t s, dim3 groups, int waves, const GemmArgs& a) {
    if (waves == 8) MMI_LAUNCH((k_gemm_xp<TN, MT, 1, 8, 4, 0, false, true>), groups, 512, 0, s, a);
    else MMI_LAUNCH((k_gemm_xp<TN, MT, 1, 4, 4, 0, false, true>), groups, 256, 0, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// k_gemm_xlds (activations resident in LDS, one workgroup per CU): which GEMMs take it, and how.  knobs.gemm_lds: '2' = with
// the staggered tail (each tile's epilogue under the last chunk's weight stream; the DEFAULT for bf16 weights at the 32-row
// tile: same-box A/B of the default benchmark 8.10 / 8.12 ms against 8.17 / 8.20 ms with k_gemm_xp, dominant kernel 38.6
// against 40.2 us live, profiles/r02_logs/ab_gemm_xlds_stagger_in_step.txt), '1' = plain tails (also what int8 / fp8 weight
// entries take when asked for; they stay on k_gemm_xp by default), '0' = k_gemm_xp everywhere.
struct XldsPlan { bool on; int kc, grid; size_t smem; bool stagger; };
XldsPlan plan_xlds(const mmi_lm* lm, const GemmW& g, const GemmArgs& a, int mt) {
    XldsPlan p{false, 0, 0, 0, false};
    const MmiKnobs& k = lm->knobs;
    const char mode = k.gemm_lds ? k.gemm_lds : (g.wq == 0 ? '2' : '0');
    if (mode == '0' || g.T != 32 || mt > 2 || g.wq == 4) return p;   // (k_gemm_xlds has no MXFP4 form)
    if (a.epi != MMI_EPI_GATE && a.epi != MMI_EPI_ROPE_KV && a.epi != MMI_EPI_STORE) return p;   // no prefetched addend, no split-K
    int cus = 256;                                             // MI355X: 256 CUs
    const bool tg = k.gemm_lds_grid != MmiKnobs::UNSET;        // test hook: small grids / short chunks for the tiny shapes
    if (k.gemm_lds_grid > 0) cus = k.gemm_lds_grid;
    const int xs = (g.wq && a.wq != 3) ? 2 : 1;                // activation fragments per weight entry (int8 activations: one entry)
    const int big = ((g.wq && a.wq != 3) ? 32 : 64) / mt;      // 64 KiB of activations per chunk buffer (int8 activations: 1 KiB per entry)
    if (g.KSTEPS % big == 0 && g.NT >= 128) p.kc = big;       // the large temporal GEMMs
    else if (tg && g.KSTEPS % 8 == 0) p.kc = 8;
    else if (tg && g.KSTEPS % 4 == 0) p.kc = 4;
    else return p;
    p.grid = g.NT < cus ? g.NT : cus;
    if (mmi_cdiv(g.NT, p.grid) > 3) return p;
    if (a.epi != MMI_EPI_GATE) {   // the kernel shares the tiles out in row octets: no workgroup may touch more than 3 tiles
        for (long b = 0; b < p.grid; ++b) {
            const long u0 = b * 4L * g.NT / p.grid, u1 = (b + 1) * 4L * g.NT / p.grid;
            if (u1 > u0 && ((u1 + 3) >> 2) - (u0 >> 2) > 3) return p;
            // a 4-bit ring's block is an octet PAIR (mmi_epi_kv_feats): every share must start on an even octet (the production
            // in_proj does: 6 octets each), else the GEMM stays on k_gemm_xp
            if (a.epi == MMI_EPI_ROPE_KV && a.kv8 == 2 && (u0 & 1)) return p;
        }
    }
    p.stagger = mode == '2' && g.wq == 0;                     // per-tile epilogues under the last chunk's stream (bf16)
    const size_t chunks = (size_t)2 * mt * p.kc * xs * 1024, red = mt == 1 ? 40960 : 65536;   // red: the epilogue's reduction scratch
    p.smem = chunks > red ? chunks : red;
    if (p.stagger && chunks < 131072) p.smem = chunks + red; // short test chunks: the scratch sits behind both buffers
    p.on = true;
    return p;
}

template <int MT, int KC, bool STAGGER, int WQ, bool KV4>
int launch_xlds_v(hipStream_t s, const XldsPlan& p, const GemmArgs& a) {
    static bool attr_set = false;
    if (!attr_set) {
        MMI_HIP_CHECK(hipFuncSetAttribute((const void*)k_gemm_xlds<MT, KC, 3, STAGGER, WQ, KV4>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
        attr_set = true;
    }
    MMI_LAUNCH((k_gemm_xlds<MT, KC, 3, STAGGER, WQ, KV4>), p.grid, 512, p.smem, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}
// production chunk (64 / MT k-steps, or 32 / MT two-step entries) or one of the short test chunks
template <int MT, bool STAGGER, int WQ, bool KV4>
int launch_xlds_kc(hipStream_t s, const XldsPlan& p, const GemmArgs& a) {
    constexpr int BIG = ((WQ == 1 || WQ == 2) ? 32 : 64) / MT;
    if (p.kc == BIG) return launch_xlds_v<MT, BIG, STAGGER, WQ, KV4>(s, p, a);
    if (p.kc == 8) return launch_xlds_v<MT, 8, STAGGER, WQ, KV4>(s, p, a);
    if (p.kc == 4) return launch_xlds_v<MT, 4, STAGGER, WQ, KV4>(s, p, a);
    return mmi_fail(MMI_ERR_UNSUPPORTED, "k_gemm_xlds: unsupported chunk");
}
template <int MT, bool KV4 = false>
int launch_xlds(hipStream_t s, const XldsPlan& p, const GemmArgs& a) {
    if (a.wq == 1) return launch_xlds_kc<MT, false, 1, KV4>(s, p, a);
    if (a.wq == 2) return launch_xlds_kc<MT, false, 2, KV4>(s, p, a);
    if (a.wq == 3) return launch_xlds_kc<MT, false, 3, KV4>(s, p, a);
    return p.stagger ? launch_xlds_kc<MT, true, 0, KV4>(s, p, a) : launch_xlds_kc<MT, false, 0, KV4>(s, p, a);
}

// k_gemm_xp_once (a wave's whole K-slice requested before its first MFMA) for the GEMMs k_gemm_xp would walk in three or more
// dependent memory round trips although they are a latency chain, not a stream: bf16 weights behind at most 256 workgroups of 8
// waves whose slice is longer than the two register buffers of k_gemm_xp (2 x 4 k-steps) and short enough for the registers -
// the depth transformer's linear_out (2816 -> 1024: 22 k-steps per wave at the 32-row tile, 11 at the 16-row tile).
// Returns the instantiated slice length, 0 = k_gemm_xp.  knobs.gemm_once '0': off (same-box A/B; bit-identical either way); 'a': every
// bf16 GEMM whose slices fit (test hook: the tiny shapes, always on 8 waves).
int once_kmax(char gemm_once, const GemmW& g, const GemmPlan& p, int mt, const GemmArgs& a) {
    const bool off = gemm_once == '0', all = gemm_once == 'a';
    if (off || a.wq != 0 || p.ntw != 1 || a.epi == MMI_EPI_GATE) return 0;
    const int kper = mmi_cdiv(mmi_cdiv(g.KSTEPS, p.ksplit), 8);
    if (!all) {
        if (p.waves != 8 || p.ksplit != 1) return 0;   // (split-K GEMMs are streams: the temporal out_proj lost 0.9 us per launch on this form)
        if ((long)g.NT * p.ksplit * (a.osplit > 1 ? a.osplit : 1) > 256) return 0;      // a stream: keep the double-buffered loop
        if (kper <= 2 * p.u) return 0;                                                   // already one round trip
    }
    if (g.T == 32 && mt == 1) return kper <= 11 ? 11 : (kper <= 22 ? 22 : 0);
    if (g.T == 16 && mt <= 2) return kper <= 11 ? 11 : 0;
    return 0;
}
template <bool KV4 = false>
int launch_once(hipStream_t s, int T, int mt, int kmax, dim3 groups, const GemmArgs& a) {
    if (T == 32 && kmax == 11) MMI_LAUNCH((k_gemm_xp_once<32, 1, 8, 11, KV4>), groups, 512, 0, s, a);
    else if (T == 32) MMI_LAUNCH((k_gemm_xp_once<32, 1, 8, 22, KV4>), groups, 512, 0, s, a);
    else if (mt == 1) MMI_LAUNCH((k_gemm_xp_once<16, 1, 8, 11, KV4>), groups, 512, 0, s, a);
    else MMI_LAUNCH((k_gemm_xp_once<16, 2, 8, 11, KV4>), groups, 512, 0, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// k_gemm_rows: more than two batch tiles of 32 (a handle of mmi_lm_create_rows, 65..128 model rows; bf16 linears).  Two n-tiles
// per workgroup once that still leaves every CU a workgroup (halves the activation bytes read from L2), else one.
// knobs.rows_ntw = 1 / 2 forces either (same-box A/B; bit-identical).
template <int MT, bool KV4>
int launch_rows_mt(hipStream_t s, int ntw, int NT, int ksplit, const GemmArgs& a) {
    const dim3 groups(mmi_cdiv(NT, ntw), ksplit);
    if (ntw == 2) MMI_LAUNCH((k_gemm_rows<32, MT, 2, 1, KV4>), groups, 256, 0, s, a);
    else MMI_LAUNCH((k_gemm_rows<32, MT, 1, 2, KV4>), groups, 256, 0, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}
template <bool KV4 = false>
int launch_rows(const MmiKnobs& k, hipStream_t s, const GemmW& g, const GemmPlan& p, int mt, const GemmArgs& a) {
    if (g.T != 32 || g.wq != 0 || a.wq != 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "more than 64 rows need bf16 linears at the 32-row tile");
    int ntw = (long)g.NT * p.ksplit >= 512 ? 2 : 1;
    if (k.rows_ntw) ntw = k.rows_ntw;
    if (mt == 3) return launch_rows_mt<3, KV4>(s, ntw, g.NT, p.ksplit, a);
    if (mt == 4) return launch_rows_mt<4, KV4>(s, ntw, g.NT, p.ksplit, a);
    return mmi_fail(MMI_ERR_UNSUPPORTED, "batch too large for the many-row GEMM");
}

// The A/B control of k_gemm_rows (knobs.rows_groups, off by default): the same GEMM as one launch of the <= 64-row kernels per
// group of two batch tiles - the weights cross HBM once per group.  GemmArgs moved to the group's rows, as
// mmi_gemm_batch_tile_view does on the device.  Only for the epilogues whose addressing is per row (store, gate, RoPE + ring).
bool rows_groups_ok(const GemmArgs& a) { return a.epi == MMI_EPI_STORE || a.epi == MMI_EPI_GATE || a.epi == MMI_EPI_ROPE_KV; }
GemmArgs rows_group_view(const GemmArgs& a_in, int r0, int rows) {
    GemmArgs a = a_in;
    a.xp += (long)(r0 / 32) * a.KSTEPS * 64;
    const long oshift = a.out_mode == MMI_OUT_PACKED ? (long)(r0 / 32) * a.out_ksteps * 512 : (long)r0 * a.out_ld;
    if (a.out) a.out += oshift;
    if (a.epi == MMI_EPI_ROPE_KV) {
        // uint16 units: an fp8 ring holds bytes, a 4-bit ring's codes plane nibbles - and its scale plane, kv_soff bytes behind the
        // codes, moves by rows of Dh / 16 bytes
        const long rows_el = (long)r0 * a.H * a.cap * a.Dh;
        const long ring = a.kv8 == 2 ? rows_el / 4 : rows_el / (a.kv8 ? 2 : 1);
        if (a.kv8 == 2) a.kv_soff += rows_el / 16 - rows_el / 2;
        a.qrot += (long)r0 * a.H * a.Dh; a.kc += ring; a.vc += ring;
        a.offsets += r0; a.rope += (long)r0 * a.Dh;
    }
    a.B = rows;
    return a;
}

// k-steps of a packed activation buffer with `features` columns (even when the linears are int8: their weight entries
// carry k-step pairs, and the padding k-step reads as zero)
int packed_ksteps_t(const mmi_lm* lm, int T, int features) {
    const int ks = mmi_cdiv(features, mmi_kstep(T));
    if (lm->q8 == 4) return 4 * mmi_cdiv(ks, 4);       // MXFP4 entries carry four k-steps
    return lm->q8 >= 1 ? 2 * mmi_cdiv(ks, 2) : ks;
}
int packed_ksteps(const mmi_lm* lm, int features) { return packed_ksteps_t(lm, lm->T, features); }
// number of bf16 elements of a packed activation buffer with `features` columns
size_t packed_elems_t(const mmi_lm* lm, int T, int features) {
    return (size_t)mmi_cdiv(lm->batch, T) * packed_ksteps_t(lm, T, features) * 512;
}
size_t packed_elems(const mmi_lm* lm, int features) { return packed_elems_t(lm, lm->T, features); }

// Where a linear writes: `features` columns, packed at the linear's tile (the operand of the next linear) or row-major with leading
// dim `features`.  GemmOut{}: the epilogue has no such output (split-K partials, the temporal in_proj's ring and q)
struct GemmOut { uint16_t* out = nullptr; int features = 0; bool packed = false; };

// THE start of every GemmArgs: all zero but the operand x (packed at tile T), the epilogue, the rows B - tok_rows sessions and
// their guidance twins - and the output geometry
GemmArgs gemm_args(const mmi_lm* lm, int T, const void* x, int epi, int B, int tok_rows, const GemmOut& o, const uint16_t* resid = nullptr) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = reinterpret_cast<const u32x4*>(x); a.out = o.out; a.resid = resid; a.epi = epi; a.B = B; a.tok_rows = tok_rows;
    a.out_mode = o.packed ? MMI_OUT_PACKED : MMI_OUT_ROWMAJOR;
    a.out_ld = o.features;
    a.out_ksteps = packed_ksteps_t(lm, T, o.features);
    return a;
}

// THE binding of a packed weight: every member of GemmArgs that is a property of the weight alone (a new weight format adds its
// members here).  wq is not: int8 activations make it a property of the launch (launch_gemm, the fused forms)
void bind_weight(GemmArgs& a, const GemmW& g) {
    a.wp = g.wp; a.N = g.N; a.KSTEPS = g.KSTEPS; a.NT = g.NT;
    a.wscale = g.scale; a.wscb = g.scb; a.ws4 = g.s4; a.gate_rows = g.gate ? g.N : 0;
    a.xinv = g.xinv;
}

// The shrink launch in front of an adapted linear g: t = bf16(A_all x) for the columns of each row's own slot (MMI_EPI_LORA_T),
// packed as the operand of g's tail.  An ordinary k_gemm_xp launch of S * R / T n-tiles over the linear's K: the waves of a
// workgroup split K as for any GEMM, and with 4..32 n-tiles the row octets of a tile are shared out (plan_osplit)
int launch_lora_shrink(mmi_lm* lm, hipStream_t s, const GemmW& g, const u32x4* xp, int B, const int* row_slot, int tok_rows, uint16_t* t) {
    auto it = lm->lora_by_wp.find(g.wp);
    if (it == lm->lora_by_wp.end()) return mmi_fail(MMI_ERR_STATE, "adapter handle: a linear without a bank");
    const int SR = lm->lora_S * lm->lora_R, mt = mmi_cdiv(B, g.T);
    GemmW ga;
    ga.wp = it->second.a; ga.N = SR; ga.K = g.K; ga.NT = SR / g.T; ga.KSTEPS = g.KSTEPS; ga.T = g.T;
    ga.bytes = (size_t)ga.NT * ga.KSTEPS * 1024;
    // (t's k-steps are whole: SR / mmi_kstep(g.T) - a slot is a multiple of 32 columns and an adapter handle's linears are bf16)
    GemmArgs a = gemm_args(lm, g.T, xp, MMI_EPI_LORA_T, B, tok_rows, {t, SR, true});
    a.wp = ga.wp; a.N = SR; a.KSTEPS = ga.KSTEPS; a.NT = ga.NT;        // a bank, not a linear of the model: no scales, no xinv
    a.row_slot = row_slot; a.lora_rank = lm->lora_R;
    const GemmPlan p = plan_gemm(lm->knobs, ga, false);
    a.osplit = plan_osplit(lm->knobs, ga, p, a.epi, g.T);
    const dim3 groups(ga.NT * (a.osplit > 1 ? a.osplit : 1), 1);
    mmi_record_bytes((long)ga.bytes);
    if (mt == 1) return g.T == 32 ? launch_lora_shrink_t<32, 1>(s, groups, p.waves, a) : launch_lora_shrink_t<16, 1>(s, groups, p.waves, a);
    if (mt == 2) return g.T == 32 ? launch_lora_shrink_t<32, 2>(s, groups, p.waves, a) : launch_lora_shrink_t<16, 2>(s, groups, p.waves, a);
    return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters run at most two batch tiles per linear");
}

// lora_t (adapter handles): the packed t of the shrink launch in front of this linear - the linear runs the LORA form of k_gemm_xp.
// An explicit argument, not a member of `a`: the lora_* members share their bytes with others (GemmArgs)
int launch_gemm(mmi_lm* lm, hipStream_t s, const GemmW& g, GemmArgs a, bool is_dominant, const u32x4* lora_t = nullptr) {
    if (lm->knobs.rows_groups && a.B > 64 && g.T == 32 && g.wq == 0 && rows_groups_ok(a)) {
        GemmArgs full = a;
        full.KSTEPS = g.KSTEPS;
        for (int r0 = 0; r0 < a.B; r0 += 64) {
            const int rc = launch_gemm(lm, s, g, rows_group_view(full, r0, a.B - r0 < 64 ? a.B - r0 : 64), is_dominant && r0 == 0);
            if (rc) return rc;
        }
        return MMI_OK;
    }
    bind_weight(a, g);                                         // (an adapter's lora_wp goes over ws4 below: bf16 linears have none)
    a.wq = (g.wq == 1 && a.wq >= 3) ? a.wq : g.wq;             // int8 linears: 3 / 4 = int8 activations (set by the program builder)
    const int mt = mmi_cdiv(a.B, g.T);
    const MmiKnobs& k = lm->knobs;
    const GemmPlan p = plan_gemm(k, g, a.epi == MMI_EPI_PARTIAL);
    // the in_proj of a 4-bit ring: the instantiations whose epilogue holds that ring form (every other launch runs the kernels it always ran)
    const bool kv4 = a.epi == MMI_EPI_ROPE_KV && a.kv8 == 2;
    a.osplit = plan_osplit(k, g, p, a.epi, g.T, kv4);
    const XldsPlan xl = plan_xlds(lm, g, a, mt);
    EvPair* ev = nullptr;
    if (lm->profiling && is_dominant) {
        if (lm->ev_used == lm->ev_pool.size()) {
            EvPair pr;
            MMI_HIP_CHECK(hipEventCreate(&pr.a));
            MMI_HIP_CHECK(hipEventCreate(&pr.b));
            lm->ev_pool.push_back(pr);
        }
        ev = &lm->ev_pool[lm->ev_used++];
        lm->prof_stream = s;
        MMI_HIP_CHECK(hipEventRecord(ev->a, s));
    }
    int rc;
    mmi_record_bytes((long)g.bytes);
    if (is_dominant) lm->dominant_xlds = xl.on && !lora_t;
    if (lora_t) {
        // an adapter handle: every linear on the LORA form of k_gemm_xp (the forms that never materialise their operand or own
        // their main loop - k_gemm_xlds, k_gemm_xp_once - are not selected; their knobs are ignored)
        auto it = lm->lora_by_wp.find(g.wp);
        if (it == lm->lora_by_wp.end() || g.wq != 0 || a.wq != 0) return mmi_fail(MMI_ERR_STATE, "adapter handle: a linear without a bank");
        a.lora_wp = it->second.b;
        a.lora_xp = lora_t;
        a.lora_ksteps = lm->lora_S * lm->lora_R / mmi_kstep(g.T);
        a.lora_slot_ksteps = lm->lora_R / mmi_kstep(g.T);
        const dim3 groups(g.NT * (a.osplit > 1 ? a.osplit : 1), p.ksplit);
        if (kv4 && mt == 1) rc = g.T == 32 ? launch_gemm_lora<32, 1, true>(s, groups, p.waves, p.u, a) : launch_gemm_lora<16, 1, true>(s, groups, p.waves, p.u, a);
        else if (kv4 && mt == 2) rc = g.T == 32 ? launch_gemm_lora<32, 2, true>(s, groups, p.waves, p.u, a) : launch_gemm_lora<16, 2, true>(s, groups, p.waves, p.u, a);
        else if (mt == 1) rc = g.T == 32 ? launch_gemm_lora<32, 1>(s, groups, p.waves, p.u, a) : launch_gemm_lora<16, 1>(s, groups, p.waves, p.u, a);
        else if (mt == 2) rc = g.T == 32 ? launch_gemm_lora<32, 2>(s, groups, p.waves, p.u, a) : launch_gemm_lora<16, 2>(s, groups, p.waves, p.u, a);
        else rc = mmi_fail(MMI_ERR_UNSUPPORTED, "adapters run at most two batch tiles per linear");
    } else if (mt > 2) {
        lm->rows_launches += 1;
        a.osplit = 1;
        rc = kv4 ? launch_rows<true>(k, s, g, p, mt, a) : launch_rows(k, s, g, p, mt, a);
    } else if (xl.on) {
        lm->xlds_launches += 1;
        if (kv4) rc = mt == 1 ? launch_xlds<1, true>(s, xl, a) : launch_xlds<2, true>(s, xl, a);
        else rc = mt == 1 ? launch_xlds<1>(s, xl, a) : launch_xlds<2>(s, xl, a);
    } else if (const int kmax = once_kmax(k.gemm_once, g, p, mt, a)) {
        const dim3 og(g.NT * (a.osplit > 1 ? a.osplit : 1), p.ksplit);
        rc = kv4 ? launch_once<true>(s, g.T, mt, kmax, og, a) : launch_once(s, g.T, mt, kmax, og, a);
    } else if (kv4) {
        rc = g.T == 32 ? launch_gemm_t<32, true>(s, p, g.NT, mt, k.q8_u2, a) : launch_gemm_t<16, true>(s, p, g.NT, mt, k.q8_u2, a);
    } else {
        rc = g.T == 32 ? launch_gemm_t<32>(s, p, g.NT, mt, k.q8_u2, a) : launch_gemm_t<16>(s, p, g.NT, mt, k.q8_u2, a);
    }
    if (rc) return rc;
    if (ev) MMI_HIP_CHECK(hipEventRecord(ev->b, s));
    return MMI_OK;
}

// int8 activations (see mmi_lm::act8)
bool act8_of(const mmi_lm* lm) { return lm->q8 == 1 && !lm->cfg.cross_attention && !lm->knobs.q8_act_bf16; }

// MMI_EPI_DEP_QKV0 (the depth transformer's in_proj at micro-step 0): where its epilogue writes k / v (frame cache, position 0)
struct DepKv { uint16_t* kc = nullptr; uint16_t* vc = nullptr; int H = 0, Dh = 0, steps = 0; };
// int8 activations of one GEMM (lm->act8): `x` is the int8 operand Xq and sx its rows' absmax (wq 3)
struct Q8 { int wq = 0; const float* sx = nullptr; };
// What an op of the step program needs beyond the weight, the operand, the epilogue and the output: a caller names the members
// its linear uses and leaves the rest alone
struct GemmOpt {
    const uint16_t* resid = nullptr;                                              // MMI_EPI_RESID: same geometry as the output
    const uint16_t* emb = nullptr; const int* tok = nullptr; int tok_stride = 0;  // MMI_EPI_EMB: the table and each session's token
    bool dominant = false;                                                        // the launch mmi_lm_profile_* times
    DepKv kv;                                                                     // MMI_EPI_DEP_QKV0
    const LmAttnArgs* ring = nullptr;      // MMI_EPI_ROPE_KV: the attention launch behind this in_proj - it reads the ring and q written here
    Q8 q8;
};

// Adapter handles: the shrink launch of linear g on its packed operand xp, as an op of its own under the site `<site>.lora`.
// Returns the packed t the linear's tail reads (launch_gemm's lora_t); null on a handle without adapters (nothing is added)
const u32x4* add_lora_shrink(mmi_lm* lm, const GemmW& g, const u32x4* xp) {
    if (!lm->lora_on) return nullptr;
    uint16_t* t = lm->lora_t;
    const std::string site = lm->prog.site_;
    lm->prog.site(site + ".lora");
    GemmW gw = g;
    const int B = lm->batch, G = lm->gen_batch;
    const int* row_slot = lm->row_slot;
    lm->prog.add([=](hipStream_t s) { return launch_lora_shrink(lm, s, gw, xp, B, row_slot, G, t); });
    lm->prog.site(site);
    return reinterpret_cast<const u32x4*>(t);
}

// One linear of the step program on the stream's rows: x = its packed operand (lm->act8: the int8 copy, with o.q8), then the
// epilogue and where it writes.  An adapter handle's shrink launch goes first, as an op of its own (add_lora_shrink)
void add_gemm(mmi_lm* lm, const GemmW& g, const void* x, int epi, const GemmOut& out, const GemmOpt& o = {}) {
    GemmArgs a = gemm_args(lm, g.T, x, epi, lm->batch, lm->gen_batch, out, o.resid);
    a.kc = o.kv.kc; a.vc = o.kv.vc; a.H = o.kv.H; a.Dh = o.kv.Dh; a.cap = o.kv.steps;
    a.wq = o.q8.wq; a.sx = o.q8.sx;
    a.emb = o.emb; a.tok = o.tok; a.tok_stride = o.tok_stride;
    if (epi == MMI_EPI_PARTIAL) a.partial = lm->partial;
    if (const LmAttnArgs* r = o.ring) {       // RoPE + ring-KV write in the epilogue
        a.qrot = r->qrot; a.kc = r->kc; a.vc = r->vc; a.offsets = r->offsets; a.H = r->H; a.Dh = r->Dh; a.cap = r->cap;
        a.max_period = r->max_period; a.rope = lm->rope; a.kv8 = lm->ring.form;
        if (a.kv8 == 2) a.kv_soff = r->kv_soff;
    }
    const u32x4* lt = add_lora_shrink(lm, g, a.xp);
    const GemmW gw = g;
    const bool dominant = o.dominant;
    lm->prog.add([lm, gw, a, dominant, lt](hipStream_t s) { return launch_gemm(lm, s, gw, a, dominant, lt); }, (long)g.bytes);
}

// The depth transformer's attention launch - the step's dep.attn op, the scoring pass and mmi_lm_debug_dep_attn: THE selection
// between the three kernels.  k_dep_attn8: a head dim that is a multiple of 8 and at most 8 positions per frame (Moshi); else the
// general one-wave-per-(row, head) kernel with 16 cache rows in registers, 32 for the TTS family's 17..32 micro-steps.
int dep_attn_kernel(int Dh, int steps) {
    if (Dh % 8 == 0 && steps <= 8) return MMI_DEP_ATTN_8;
    return steps > 16 ? MMI_DEP_ATTN_ROWS32 : MMI_DEP_ATTN_ROWS16;
}
// force: MMI_DEP_ATTN_AUTO, or (the tap alone) a kernel that admits the shape; ran: the kernel launched, when asked for
int launch_dep_attn(hipStream_t s, const DepAttnArgs& da, int force = MMI_DEP_ATTN_AUTO, int* ran = nullptr) {
    const int kernel = force == MMI_DEP_ATTN_AUTO ? dep_attn_kernel(da.Dh, da.steps) : force;
    if (kernel == MMI_DEP_ATTN_8) MMI_LAUNCH((k_dep_attn8<4>), mmi_cdiv(da.B * da.H, 4), 256, 0, s, da);
    else if (kernel == MMI_DEP_ATTN_ROWS32) MMI_LAUNCH((k_dep_attn<32>), da.B * da.H, 64, 0, s, da);
    else MMI_LAUNCH((k_dep_attn<16>), da.B * da.H, 64, 0, s, da);
    MMI_CHECK_LAUNCH();
    if (ran) *ran = kernel;
    return MMI_OK;
}

// The L.cross_attn op (and mmi_lm_debug_cross_attn)
int launch_cross_attn(hipStream_t s, const CrossAttnArgs& ca) {
    MMI_LAUNCH(k_lm_cross_attn, ca.B * ca.H, 64, 0, s, ca);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// The depth transformer's attention inside its out_proj (k_dep_attn_out_proj): ONE session at the 16-row tile (the real-time
// configuration), bf16 weights, a wave's K-slice = one or two whole heads.  Same-box at 1 / 2 / 4 sessions: -0.06 / +0.04 / +0.27 ms
// per step (a wave works through its 2 B pairs one after the other; profiles/r04_logs/call_o2_summary.txt), hence one session only.
// knobs.no_dep_attn_fusion: the two launches (A/B and the bit-equality test).  A function of the weight, the shape and the rows
// (the step: its streaming batch; mmi_lm_debug_dep_attn_out_proj: 1) - nothing of a running stream.
bool dep_attn_fusable(const mmi_lm* lm, const GemmW& g, int H, int Dh, int steps, int rows) {
    if (g.T != 16 || rows != 1 || lm->act8 || g.wq != 0 || lm->knobs.no_dep_attn_fusion || lm->lora_on) return false;
    if (Dh % 8 || Dh > 64 || steps > 8 || g.KSTEPS * 32 != H * Dh) return false;
    const GemmPlan p = plan_gemm(lm->knobs, g, false);
    const int kper = mmi_cdiv(g.KSTEPS, p.waves);
    return kper <= 4 && (kper * 32) % Dh == 0 && kper * 32 / Dh <= 2;
}

template <int WAVES>
int launch_dep_attn_out_proj(hipStream_t s, int groups, const GemmArgs& a, const DepAttnArgs& d) {
    MMI_LAUNCH((k_dep_attn_out_proj<WAVES, 2, 1>), groups, WAVES * 64, 0, s, a, d);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// x += out_proj(attention(qkv, frame cache)) (dep_attn_fusable)
// the fused launch with its plan (the step's op and mmi_lm_debug_dep_attn_out_proj): B = tok_rows = 1 (dep_attn_fusable)
struct DepAttnOutProj { GemmArgs a; int groups, waves; };
DepAttnOutProj plan_dep_attn_out_proj(const mmi_lm* lm, const GemmW& g, uint16_t* x, int features, int B, int tok_rows) {
    DepAttnOutProj f;
    GemmArgs& a = f.a;
    a = gemm_args(lm, g.T, nullptr, MMI_EPI_RESID, B, tok_rows, {x, features, true}, x);     // (the operand is the attention's, in registers)
    bind_weight(a, g);
    const GemmPlan p = plan_gemm(lm->knobs, g, false);
    a.osplit = plan_osplit(lm->knobs, g, p, a.epi, g.T);
    f.groups = g.NT * (a.osplit > 1 ? a.osplit : 1);
    f.waves = p.waves;
    return f;
}
int launch_dep_attn_out_proj_planned(hipStream_t s, const DepAttnOutProj& f, const DepAttnArgs& da) {
    return f.waves == 8 ? launch_dep_attn_out_proj<8>(s, f.groups, f.a, da) : launch_dep_attn_out_proj<4>(s, f.groups, f.a, da);
}
void add_dep_attn_out_proj(mmi_lm* lm, const GemmW& g, const DepAttnArgs& da, uint16_t* x, int features) {
    const DepAttnOutProj f = plan_dep_attn_out_proj(lm, g, x, features, lm->batch, lm->gen_batch);
    const long bytes = (long)g.bytes;
    lm->prog.add([=](hipStream_t s) {
        mmi_record_bytes(bytes);
        return launch_dep_attn_out_proj_planned(s, f, da);
    }, bytes);
}

// The split-K partials a norm launch still has to fold into the residual stream: P of them; int8 x int8 GEMMs leave int32 sums
// and the norm dequantises (sx = the absmax of the GEMM's input rows, scb = its SCB; k_resid_rmsnorm psx / pscb)
struct Pending { int P = 0; const float* sx = nullptr; const float* scb = nullptr; };

// K-split GEMM whose partial sums (lm->partial) the following add_resid_rmsnorm folds into the residual stream.
// Returns the partials, P = 0 when the GEMM is not split (then it applied the residual itself, in place on x).
Pending add_gemm_resid(mmi_lm* lm, const GemmW& g, const void* in, uint16_t* x, int features, Q8 q8 = {}) {
    const GemmPlan p = plan_gemm(lm->knobs, g, true);
    GemmOpt o;
    o.q8 = q8;
    if (p.ksplit <= 1) {
        o.resid = x;
        add_gemm(lm, g, in, MMI_EPI_RESID, {x, features, true}, o);
        return Pending{};
    }
    add_gemm(lm, g, in, MMI_EPI_PARTIAL, {}, o);
    Pending pd;
    pd.P = p.ksplit;
    if (q8.wq == 3 && g.wq == 1) { pd.sx = q8.sx; pd.scb = g.scb; }
    return pd;
}

// threads of a launch with one workgroup per row of D features: one 16-byte piece per thread where the row allows it
int row_threads(int D) {
    const int nth = mmi_cdiv(D / 8, 64) * 64;
    return nth > 1024 ? 1024 : nth;
}

// THE launch of k_resid_rmsnorm: x (+= the pending split-K partials, held in `partial`), y = rms_norm(x) * alpha, rows packed at
// `tile` with `ksteps` k-steps.  yq / sx: also store the row quantised row-wise to int8 (+ its absmax) for the int8 linears that
// read it (lm->act8)
int launch_rmsnorm(hipStream_t s, int rows, uint16_t* x, const float* partial, Pending pd, const uint16_t* alpha, uint16_t* y, int D, int tile,
                   int ksteps, uint8_t* yq = nullptr, float* sx = nullptr) {
    MMI_LAUNCH(k_resid_rmsnorm, rows, row_threads(D), 0, s, x, partial, pd.P, rows, alpha, y, D, tile, ksteps, 1e-8f, yq, sx, pd.sx, pd.scb);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

void add_resid_rmsnorm(mmi_lm* lm, uint16_t* x, Pending pd, const uint16_t* alpha, uint16_t* y, int D, uint8_t* yq = nullptr, float* sx = nullptr,
                       int tile = 0) {
    const int B = lm->batch, T = tile ? tile : lm->T, ksteps = packed_ksteps_t(lm, T, D);
    const float* partial = lm->partial;
    lm->prog.add([=](hipStream_t s) { return launch_rmsnorm(s, B, x, partial, pd, alpha, y, D, T, ksteps, yq, sx); });
}

// parity tap (mmi_lm_set_hidden_taps; off in production: no op is added): the residual stream, row-major, into htap[which]
void add_hidden_tap(mmi_lm* lm, int which) {
    if (!lm->htap) return;
    const int B = lm->batch, d = lm->cfg.dim, T = lm->T, ksteps = packed_ksteps(lm, d);
    const uint16_t* x = lm->x;
    uint16_t* dst = lm->htap + (size_t)which * B * d;
    lm->prog.add([=](hipStream_t s) {
        MMI_LAUNCH(k_unpack_rows, mmi_cdiv(B * d, 256), 256, 0, s, x, B, d, dst, T, ksteps);
        MMI_CHECK_LAUNCH();
        return (int)MMI_OK;
    });
}

// RMSNorm fused in front of a short-row GEMM (k_gemm_xp_norm; int8 x int8: k_gemm_q8<NORM>): the launch by tile / batch tiles / weight format
// tiles_over_grid (k_gemm_q8 at 33..64 sessions): one batch tile per workgroup (grid.y = tiles; the default) or both tiles walked by
// one workgroup (knobs.q8_tiles_serial: the round-4 form, same-box A/B)
int launch_norm_fused(hipStream_t s, int T, int mt, int wq, int NT, bool tiles_over_grid, const GemmArgs& a) {
    if (wq == 1) {
        if (T == 32 && mt == 1) MMI_LAUNCH((k_gemm_xp_norm<32, 1, 8, 4, 1>), NT, 512, 0, s, a);
        else if (T == 32) MMI_LAUNCH((k_gemm_xp_norm<32, 2, 8, 4, 1>), NT, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_xp_norm<16, 1, 8, 4, 1>), NT, 512, 0, s, a);
    } else if (wq == 3) {
        if (T == 32 && mt == 1) MMI_LAUNCH((k_gemm_q8<32, 1, 8, 4, true>), NT, 512, 0, s, a);
        else if (T == 32 && tiles_over_grid) MMI_LAUNCH((k_gemm_q8<32, 1, 8, 4, true>), dim3(NT, mt), 512, 0, s, a);
        else if (T == 32) MMI_LAUNCH((k_gemm_q8<32, 2, 8, 4, true>), NT, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_q8<16, 1, 8, 4, true>), NT, 512, 0, s, a);
    } else if (wq == 4) {      // rows of <= 16 entries: two per wave
        if (T == 32 && mt == 1) MMI_LAUNCH((k_gemm_xp_norm<32, 1, 8, 2, 4>), NT, 512, 0, s, a);
        else if (T == 32) MMI_LAUNCH((k_gemm_xp_norm<32, 2, 8, 2, 4>), NT, 512, 0, s, a);
        else if (mt == 1) MMI_LAUNCH((k_gemm_xp_norm<16, 1, 8, 2, 4>), NT, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_xp_norm<16, 2, 8, 2, 4>), NT, 512, 0, s, a);
    } else if (wq == 2) {
        if (T == 32 && mt == 1) MMI_LAUNCH((k_gemm_xp_norm<32, 1, 8, 4, 2>), NT, 512, 0, s, a);
        else if (T == 32) MMI_LAUNCH((k_gemm_xp_norm<32, 2, 8, 4, 2>), NT, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_xp_norm<16, 1, 8, 4, 2>), NT, 512, 0, s, a);
    } else {
        if (T == 32 && mt == 1) MMI_LAUNCH((k_gemm_xp_norm<32, 1, 8, 8>), NT, 512, 0, s, a);
        else if (T == 32) MMI_LAUNCH((k_gemm_xp_norm<32, 2, 8, 8>), NT, 512, 0, s, a);
        // 16-row tile: rows of <= 32 k-steps (the depth transformer's 1024 features) need 4 fragments per wave, not 8: the
        // smaller register arrays let two workgroups share a CU, so the 352 gated tiles of linear_in are resident at once
        // instead of running as 256 + 96 (same k partition per wave: bit-identical)
        else if (mt == 2 && a.KSTEPS <= 32) MMI_LAUNCH((k_gemm_xp_norm<16, 2, 8, 4>), NT, 512, 0, s, a);   // 17..32 sessions on the depth
        else if (mt == 2) MMI_LAUNCH((k_gemm_xp_norm<16, 2, 8, 8>), NT, 512, 0, s, a);                      // transformer's own tile (lm->Td)
        else if (a.KSTEPS <= 32) MMI_LAUNCH((k_gemm_xp_norm<16, 1, 8, 4>), NT, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_xp_norm<16, 1, 8, 8>), NT, 512, 0, s, a);
    }
    MMI_CHECK_LAUNCH();
    return (int)MMI_OK;
}

// k_gemm_q8 without a norm: the row quantisation inside the GEMM (kmax = 4: rows of <= 32 entries, 11: <= 88)
int launch_q8_fused(hipStream_t s, int T, int mt, int kmax, int NT, bool tiles_over_grid, const GemmArgs& a) {
    if (kmax == 4) {
        if (T == 32 && mt == 1) MMI_LAUNCH((k_gemm_q8<32, 1, 8, 4, false>), NT, 512, 0, s, a);
        else if (T == 32 && tiles_over_grid) MMI_LAUNCH((k_gemm_q8<32, 1, 8, 4, false>), dim3(NT, mt), 512, 0, s, a);
        else if (T == 32) MMI_LAUNCH((k_gemm_q8<32, 2, 8, 4, false>), NT, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_q8<16, 1, 8, 4, false>), NT, 512, 0, s, a);
    } else {
        if (T == 32 && mt == 1) MMI_LAUNCH((k_gemm_q8<32, 1, 8, 11, false>), NT, 512, 0, s, a);
        else if (T == 32 && tiles_over_grid) MMI_LAUNCH((k_gemm_q8<32, 1, 8, 11, false>), dim3(NT, mt), 512, 0, s, a);
        else if (T == 32) MMI_LAUNCH((k_gemm_q8<32, 2, 8, 11, false>), NT, 512, 0, s, a);
        else MMI_LAUNCH((k_gemm_q8<16, 1, 8, 11, false>), NT, 512, 0, s, a);
    }
    MMI_CHECK_LAUNCH();
    return (int)MMI_OK;
}
static int q8_fused_kmax(const GemmW& g) { return g.KSTEPS <= 32 ? 4 : (g.KSTEPS <= 88 ? 11 : 0); }
static int q8_fused_osplit(const MmiKnobs& k, const GemmW& g, int epi, int T) {
    int os = 1;
    if (epi != MMI_EPI_GATE && !k.gemm_osplit_set) {
        const int octs = T / 8;
        while (os < octs && (long)g.NT * os < 128) os *= 2;
        if (g.NT > 64) os = 1;
    }
    return os;
}

// longest row (in weight entries) of the norm-fused GEMM: 8 waves x 8 k-steps
static int norm_fused_max(int wq) { return wq == 4 ? 16 : (wq ? 32 : 64); }

// RMSNorm(x) * alpha fused into the GEMM (k_gemm_xp_norm) when a workgroup's 8 waves can hold the whole row slice in
// registers (rows of <= 1024 features at the 32-wide tile: the depth transformer); otherwise norm kernel + GEMM.
// lm->act8: the normalised row is quantised inside the GEMM (k_gemm_q8, fused) or by the norm launch
void add_norm_gemm(mmi_lm* lm, const GemmW& g, uint16_t* x, const uint16_t* alpha, uint16_t* xn_scratch, int D, int epi, const GemmOut& out,
                   const DepKv& kv = {}) {
    const bool a8 = lm->act8 && g.wq == 1;
    const int wq = a8 ? 3 : g.wq;
    const bool fuse = g.KSTEPS <= norm_fused_max(wq) && !lm->knobs.no_norm_fusion && mmi_cdiv(lm->batch, g.T) <= 2 &&   // k_gemm_rows has no fused norm
                      !lm->lora_on;                            // an adapter's shrink launch reads the materialised operand
    if (!fuse) {
        GemmOpt o;
        o.kv = kv;
        if (a8) o.q8 = Q8{3, lm->sx_dxn};
        add_resid_rmsnorm(lm, x, Pending{}, alpha, xn_scratch, D, a8 ? lm->dxnq : nullptr, a8 ? lm->sx_dxn : nullptr, g.T);
        add_gemm(lm, g, a8 ? (const void*)lm->dxnq : xn_scratch, epi, out, o);
        return;
    }
    GemmArgs a = gemm_args(lm, g.T, x, epi, lm->batch, lm->gen_batch, out);
    a.kc = kv.kc; a.vc = kv.vc; a.H = kv.H; a.Dh = kv.Dh; a.cap = kv.steps;
    a.alpha = alpha; a.D = D; a.eps = 1e-8f;
    bind_weight(a, g);
    a.wq = wq;
    a.osplit = 1;
    const int T = g.T, mt = mmi_cdiv(lm->batch, g.T), NT = g.NT * (a.osplit > 1 ? a.osplit : 1);
    const long gbytes = (long)g.bytes;
    const bool over_grid = !lm->knobs.q8_tiles_serial;
    lm->prog.add([=](hipStream_t s) {
        mmi_record_bytes(gbytes);
        return launch_norm_fused(s, T, mt, wq, NT, over_grid, a);
    }, gbytes);
}

// bf16 packed tensor -> its row-wise int8 copy + the rows' absmax (lm->act8): one workgroup per row
void add_quant_rows(mmi_lm* lm, const uint16_t* xp, uint8_t* xq, float* sx, int features, int tile = 0) {
    const int B = lm->batch, T = tile ? tile : lm->T, ksteps = packed_ksteps_t(lm, T, features);
    lm->prog.add([=](hipStream_t s) {
        MMI_LAUNCH(k_quant_rows_i8, B, row_threads(features), 0, s, xp, B, features, T, ksteps, xq, sx);
        MMI_CHECK_LAUNCH();
        return (int)MMI_OK;
    });
}

// An int8 linear of the depth transformer on a bf16 input WITHOUT a norm in front (out_proj, linear_out, the logits heads) under
// lm->act8: the row quantisation fused into the GEMM (k_gemm_q8, rows of <= 8 * 11 entries); longer rows: quantisation launch
// (into the gated tensor's scratch) + the plain int8 x int8 GEMM.
void add_q8_gemm(mmi_lm* lm, const GemmW& g, const uint16_t* x, int in_features, int epi, const GemmOut& out, const uint16_t* resid = nullptr) {
    const int T = g.T, mt = mmi_cdiv(lm->batch, g.T);
    const int kmax = q8_fused_kmax(g);
    if (!kmax || lm->knobs.no_norm_fusion) {
        add_quant_rows(lm, x, lm->hbq, lm->sx_hb, in_features, g.T);
        GemmOpt o;
        o.resid = resid;
        o.q8 = Q8{3, lm->sx_hb};
        add_gemm(lm, g, lm->hbq, epi, out, o);
        return;
    }
    GemmArgs a = gemm_args(lm, g.T, x, epi, lm->batch, lm->gen_batch, out, resid);
    bind_weight(a, g);
    a.wq = 3;
    // few n-tiles (the N = 1024 linears: 32 tiles for 256 CUs): share a tile's row octets out over several workgroups, as
    // plan_osplit does for the bf16 form of these GEMMs
    a.osplit = q8_fused_osplit(lm->knobs, g, epi, T);
    const int NT = g.NT * a.osplit;
    const long gbytes = (long)g.bytes;
    const bool over_grid = !lm->knobs.q8_tiles_serial;
    lm->prog.add([=](hipStream_t s) {
        mmi_record_bytes(gbytes);
        return launch_q8_fused(s, T, mt, kmax, NT, over_grid, a);
    }, gbytes);
}

// next_k >= 0: the sampled token opens depth-transformer micro-step next_k, whose input row the sampler writes itself
void add_sample(mmi_lm* lm, uint16_t* logits, int ld, int V, bool text, int site, int* out, int out_stride, int next_k = -1) {
    const bool guided = lm->cfg_coef != 1.f;
    if (guided && !(text && lm->cfg_no_text)) {     // lm.py:727-733 (text; `cfg_is_no_text` keeps the conditioned logits), 828-832
        const int G = lm->gen_batch;
        const float* coefs = lm->coefs;
        lm->prog.add([=](hipStream_t s) {
            MMI_LAUNCH(k_cfg_mix, dim3(mmi_cdiv(V, 256), G), 256, 0, s, logits, ld, V, G, coefs);
            MMI_CHECK_LAUNCH();
            return (int)MMI_OK;
        });
    }
    SampleArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.nx_dup = guided ? lm->gen_batch : 0;
    if (next_k >= 0) {
        const int dd = lm->cfg.depformer_dim;
        sa.nx_pre = lm->dpre + (size_t)lm->dep_sched[next_k] * dd; sa.nx_ld = lm->dep_nw * dd;
        sa.nx_emb = lm->dep_emb[next_k]; sa.nx_out = lm->dx;
        sa.nx_D = dd; sa.nx_T = lm->Td; sa.nx_ksteps = packed_ksteps_t(lm, lm->Td, dd);
    }
    sa.logits = logits; sa.ld = ld; sa.V = V;
    sa.k = text ? lm->samp.top_k_text : lm->samp.top_k;
    sa.temp = text ? lm->samp.temp_text : lm->samp.temp;
    sa.use_sampling = lm->samp.use_sampling;
    if (sa.k >= V) sa.k = 0;   // top_k == 0 (or the whole vocabulary): plain multinomial, k_sample's a.k <= 0 branch
    sa.noise = lm->noise + (size_t)site * lm->kmax;
    sa.noise_ld = (1 + lm->cfg.dep_q) * lm->kmax;
    sa.use_noise = lm->use_noise; sa.rng = lm->rng; sa.site = site; sa.out = out; sa.out_stride = out_stride;
    sa.B = lm->gen_batch;
    sa.forced = lm->forced + site; sa.forced_stride = 1 + lm->cfg.dep_q; sa.use_forced = lm->use_forced;
    sa.rows = lm->rowtab; sa.offsets = lm->offsets; sa.thist = text ? lm->thist : nullptr; sa.text = text ? 1 : 0;
    sa.pad_id = lm->cfg.existing_text_padding_id;
    if (text && lm->tts) { sa.bonus_id = lm->tts_p.pad; sa.bonus = lm->tts_p.padding_bonus; }
    const int B = lm->gen_batch;
    if (text) {                     // hook boundaries: the guided logits are final here, the sampler is the next op
        lm->op_text_sample = lm->prog.ops.size();
        lm->op_after_text_sample = lm->op_text_sample + 1;
        lm->text_sample_args = sa;
    }
    if (lm->nucleus_on) {           // the nucleus forms of the same three geometries (mmi_lm_enable_nucleus)
        lm->prog.add([=](hipStream_t s) {
            if (V <= 2048) MMI_LAUNCH((k_sample_nucleus<256, 8>), B, 256, 0, s, sa);
            else if (V <= 8192) MMI_LAUNCH((k_sample_nucleus<1024, 8>), B, 1024, 0, s, sa);
            else MMI_LAUNCH((k_sample_nucleus<1024, 32>), B, 1024, 0, s, sa);
            MMI_CHECK_LAUNCH();
            return (int)MMI_OK;
        });
        return;
    }
    lm->prog.add([=](hipStream_t s) {
        if (V <= 2048) MMI_LAUNCH((k_sample<256, 8, true>), B, 256, 0, s, sa);
        else if (V <= 8192) MMI_LAUNCH((k_sample<1024, 8, true>), B, 1024, 0, s, sa);
        else MMI_LAUNCH((k_sample<1024, 32, true>), B, 1024, 0, s, sa);   // 32 logits per thread = 16 VGPRs: read once, not once per pass
        MMI_CHECK_LAUNCH();
        return (int)MMI_OK;
    });
}

// the default since round 4: k_lm_attn_wave, one online softmax per wave, no barrier in the loop; knobs.attn_split = the chunked
// kernel of rounds 1-3 (same-box A/Bs)
static bool attn_wave_kernel(const MmiKnobs& k) { return !k.attn_split; }

// workgroups per (session, head) of the decode attention.  k_lm_attn_wave: ONE from 128 pairs (4 sessions) on - one workgroup per
// pair walking the whole ring beats ring split + merge launch at every depth there (4 / 8 / 16 sessions, 3000 rows: -0.03 / -0.16 /
// -0.16 ms per step, profiles/r04_logs/call_v_summary.txt); below that the ring is split (and still walked by one workgroup while
// it is short: attn_solo_rows).  The chunked kernel of rounds 1-3: 1 once B*H alone fills the chip.
int attn_splits(const MmiKnobs& k, const mmi_lm_cfg& c, int B) {
    if (k.attn_ns) return k.attn_ns;                      // test hook: the split + combine path on rings too short to need it
    if (attn_wave_kernel(k) && B * c.num_heads >= 128) return 1;
    const int chunks = mmi_cdiv(c.context, MMI_ATTN_CHUNK);
    int want = 1024 / (B * c.num_heads);
    if (want < 1) want = 1;
    return want < chunks ? want : chunks;
}

// k_lm_attn_wave, ring split over several workgroups: up to this many rows, workgroup 0 walks the ring alone and writes the output
// itself.  Measured crossover against split + merge launch (profiles/r04_logs/call_u_summary.txt, call_v_summary.txt): one session
// between 600 and 900 rows, two sessions between 600 and 1800.  knobs.attn_solo: test hook (0 = always the merge launch)
static int attn_solo_rows(const MmiKnobs& k, int pairs) {
    if (k.attn_solo != MmiKnobs::UNSET) return k.attn_solo;
    return pairs <= 32 ? 768 : 1200;
}

// The ring split over NS > 1 workgroups (fewer than 32 sessions) has two step programs (MmiProgram::variant):
//   0  while no ring can hold more than solo_rows rows (the host's bound on the offsets): k_lm_attn_wave alone - workgroup 0 of
//      each (session, head) walks the ring and writes the output.  One launch per layer instead of two: 4.4 us x 32 layers of a
//      4.7 ms single-session step.  (Should a ring be longer all the same, the kernel merges in its last-arriving workgroup:
//      correct whatever the host believes, 8 us per layer slower than a launch - measured, profiles/r04_logs/call_j_summary.txt)
//   1  deeper rings: partials from every workgroup + the k_lm_attn_combine launch, as in rounds 1-3.
// knobs.attn_merge_kernel (test hook) stays on variant 0 whatever the depth.
static int attn_variant(const mmi_lm* lm, int NS) {
    if (NS <= 1 || !attn_wave_kernel(lm->knobs) || lm->knobs.attn_merge_kernel) return 0;
    return lm->depth_bound + 1 > (long)attn_solo_rows(lm->knobs, lm->batch * lm->cfg.num_heads) ? 1 : 0;
}

// One layer's ring in uint16 units, keys or values.  bf16: an element each; e4m3: a byte each; 4-bit (MMI_F4E2M1X2): the codes
// plane [B][H][cap][Dh/2] bytes, then the scale plane [B][H][cap][Dh/16] bytes - 9/16 of a byte per element (Dh % 32 == 0).
static int kv_form(int32_t kv_cache_dtype) { return kv_cache_dtype == MMI_F8E4M3 ? 1 : (kv_cache_dtype == MMI_F4E2M1X2 ? 2 : 0); }
// The 4-bit layer is padded to a multiple of 256 bytes, so that the next layer's codes plane starts 16-byte aligned whatever the
// capacity (the scale plane is a multiple of 2 bytes only); the other rings are as they were.
static size_t kv_layer_u16(int kvf, size_t elems) { return kvf == 2 ? (elems / 4 + elems / 32 + 127) / 128 * 128 : elems / (kvf ? 2 : 1); }
// The ring of a stream of B model rows: the one place that derives it from the configuration (mmi_lm::ring)
static KvRing kv_ring_of(const mmi_lm_cfg& c, int B) {
    KvRing r;
    r.form = kv_form(c.kv_cache_dtype);
    r.elems = (size_t)B * c.num_heads * c.context * (c.dim / c.num_heads);
    r.layer_u16 = kv_layer_u16(r.form, r.elems);
    r.codes_bytes = r.form == 2 ? r.elems / 2 : r.elems * (r.form ? 1 : 2);
    r.scale_off = r.form == 2 ? r.codes_bytes : 0;
    return r;
}

// kvf: the ring form (kv_form).  The bf16 and e4m3 launches are spelled as they always were: the spelling is the kernel's name in
// mmi_lm_launch_list
int launch_attn_split(hipStream_t s, const LmAttnArgs& a, int kvf, bool wave) {
    dim3 grid(a.B * a.H, a.NS);
    const bool kv8 = kvf == 1;
    if (kvf == 2) {
        if (wave) {
            switch (a.Dh) {
                case 128: MMI_LAUNCH((k_lm_attn_wave<128, 2>), grid, 256, 0, s, a); break;
                case 64: MMI_LAUNCH((k_lm_attn_wave<64, 2>), grid, 256, 0, s, a); break;
                case 32: MMI_LAUNCH((k_lm_attn_wave<32, 2>), grid, 256, 0, s, a); break;
                default: return mmi_fail(MMI_ERR_UNSUPPORTED, "head dim must be 32, 64 or 128");
            }
        } else {
            switch (a.Dh) {
                case 128: MMI_LAUNCH((k_lm_attn_split<128, 2>), grid, 256, 0, s, a); break;
                case 64: MMI_LAUNCH((k_lm_attn_split<64, 2>), grid, 256, 0, s, a); break;
                case 32: MMI_LAUNCH((k_lm_attn_split<32, 2>), grid, 256, 0, s, a); break;
                default: return mmi_fail(MMI_ERR_UNSUPPORTED, "head dim must be 32, 64 or 128");
            }
        }
        MMI_CHECK_LAUNCH();
        return MMI_OK;
    }
    if (wave) {
        if (kv8) {
            switch (a.Dh) {
                case 128: MMI_LAUNCH((k_lm_attn_wave<128, true>), grid, 256, 0, s, a); break;
                case 64: MMI_LAUNCH((k_lm_attn_wave<64, true>), grid, 256, 0, s, a); break;
                case 32: MMI_LAUNCH((k_lm_attn_wave<32, true>), grid, 256, 0, s, a); break;
                default: return mmi_fail(MMI_ERR_UNSUPPORTED, "head dim must be 32, 64 or 128");
            }
        } else {
            switch (a.Dh) {
                case 128: MMI_LAUNCH((k_lm_attn_wave<128>), grid, 256, 0, s, a); break;
                case 64: MMI_LAUNCH((k_lm_attn_wave<64>), grid, 256, 0, s, a); break;
                case 32: MMI_LAUNCH((k_lm_attn_wave<32>), grid, 256, 0, s, a); break;
                default: return mmi_fail(MMI_ERR_UNSUPPORTED, "head dim must be 32, 64 or 128");
            }
        }
        MMI_CHECK_LAUNCH();
        return MMI_OK;
    }
    if (kv8) {
        switch (a.Dh) {
            case 128: MMI_LAUNCH((k_lm_attn_split<128, true>), grid, 256, 0, s, a); break;
            case 64: MMI_LAUNCH((k_lm_attn_split<64, true>), grid, 256, 0, s, a); break;
            case 32: MMI_LAUNCH((k_lm_attn_split<32, true>), grid, 256, 0, s, a); break;
            default: return mmi_fail(MMI_ERR_UNSUPPORTED, "head dim must be 32, 64 or 128");
        }
        MMI_CHECK_LAUNCH();
        return MMI_OK;
    }
    switch (a.Dh) {
        case 128: MMI_LAUNCH((k_lm_attn_split<128>), grid, 256, 0, s, a); break;
        case 64: MMI_LAUNCH((k_lm_attn_split<64>), grid, 256, 0, s, a); break;
        case 32: MMI_LAUNCH((k_lm_attn_split<32>), grid, 256, 0, s, a); break;
        default: return mmi_fail(MMI_ERR_UNSUPPORTED, "head dim must be 32, 64 or 128");
    }
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// The L.attn op (and mmi_lm_debug_attn): the attention launch and, with merge_launch, the merge of the workgroups' partials as a
// launch of its own
int launch_attn(hipStream_t s, const LmAttnArgs& a, int kvf, bool wave, bool merge_launch) {
    LmAttnArgs aa = a;
    if (merge_launch) { aa.solo_rows = -1; aa.done = nullptr; }     // every workgroup leaves its partial (m, l, O)
    int rc = launch_attn_split(s, aa, kvf, wave);
    if (rc) return rc;
    if (merge_launch) MMI_LAUNCH(k_lm_attn_combine, aa.B * aa.H, aa.Dh < 64 ? 64 : aa.Dh, 0, s, aa);
    MMI_CHECK_LAUNCH();
    return (int)MMI_OK;
}

TokArgs tok_args(mmi_lm* lm) {
    TokArgs t;
    t.cache = lm->cache; t.offsets = lm->offsets; t.exec = lm->exec; t.delays = lm->delays_dev;
    t.B = lm->gen_batch; t.NC = lm->NC; t.CT = lm->CT; t.dep_q = lm->cfg.dep_q; t.max_delay = lm->max_delay;
    t.card = lm->cfg.card; t.text_card = lm->cfg.text_card;
    t.rows = lm->rowtab; t.thist = lm->thist;
    t.text_pad = lm->cfg.existing_text_padding_id; t.text_eop = lm->text_eop;      // LMModel.end_of_text_padding_id (lm.py:261); gen.rs:79
    t.tts = lm->tts; t.tts_stride = lm->tts_stride; t.tts_max_prefix = lm->tts_max_prefix;
    t.tts_aprefix = MMI_TTS_HDR + 2 * lm->tts_max_tokens + 3 * lm->tts_max_entries + 1 + lm->tts_max_prefix;
    t.tts_zero = lm->tts_p.zero; t.tts_delay_steps = lm->tts_p.delay_steps; t.tts_initial_padding = lm->tts_p.initial_padding;
    t.tts_audio = lm->tts ? 1 : 0;
    return t;
}

// k_step_logprob: the op of the step program (and mmi_lm_debug_step_logprob, on caller rows)
int launch_step_logprob(hipStream_t s, const LpArgs& a, int rows) {
    MMI_LAUNCH(k_step_logprob, dim3(rows, a.r.sites), MMI_SCORE_THREADS, 0, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

LpArgs step_logprob_args(mmi_lm* lm) {
    const mmi_lm_cfg& c = lm->cfg;
    LpArgs a;
    memset(&a, 0, sizeof(a));
    a.t = tok_args(lm);
    a.text_logits = lm->text_logits; a.text_N = c.text_card_out;
    a.dlogits = lm->dlogits; a.dstride = (long)lm->batch * c.card; a.card = c.card;
    a.text_tok = lm->text_tok; a.audio_tok = lm->audio_tok;
    a.r = lm->lp;
    return a;
}

// the rings of the stream's rows back to NaN / -1: by mmi_lm_reset's device mask (null = every row), or the n rows `sess`
int clear_logprobs(mmi_lm* lm, hipStream_t s, const uint8_t* mask, const uint8_t* sess = nullptr, int n = -1) {
    if (!lm->lp.lp) return MMI_OK;
    LpClear c;
    memset(&c, 0, sizeof(c));
    c.r = lm->lp; c.CT = lm->CT; c.n = n; c.mask = mask;
    if (n > 0) memcpy(c.sess, sess, (size_t)n);
    MMI_LAUNCH(k_lp_clear, n >= 0 ? n : lm->gen_batch, 256, 0, s, c);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

int build_program(mmi_lm* lm) {
    const mmi_lm_cfg& c = lm->cfg;
    const int B = lm->batch, d = c.dim, H = c.num_heads, Dh = d / H;
    const int dd = c.depformer_dim, Hd = c.depformer_num_heads, Dhd = dd / Hd;
    const int n_user = c.n_q - c.dep_q;
    MmiProgram& P = lm->prog;
    const bool a8 = lm->act8;
    // ---- token ring in, embeddings
    P.site("prepare");
    {
        TokArgs t = tok_args(lm);
        const int* user = lm->user_i32; int* tokens = lm->tokens;
        const uint16_t *emb = lm->emb, *temb = lm->text_emb; uint16_t* x = lm->x; const int NC = lm->NC, card1 = c.card + 1;
        const int T = lm->T, xks = packed_ksteps(lm, d);
        float* rope = lm->rope; const float max_period = c.max_period;
        const int G = lm->gen_batch;
        const bool guided = lm->cfg_coef != 1.f;
        const int* masked_until = lm->masked_until; const int no_text = lm->cfg_no_text; long* offsets_m = lm->offsets_m;
        const uint16_t* cond = lm->cond;
        const uint16_t* temb2 = lm->demux ? lm->text_emb2 : nullptr; const int text_n = c.text_card + 1;
        P.add([=](hipStream_t s) {
            MMI_LAUNCH(k_lm_prepare, mmi_cdiv(G * NC + G * (Dh / 2), 128), 128, 0, s, t, user, n_user, tokens, rope, Dh, max_period);
            if (guided)
                MMI_LAUNCH(k_lm_cfg_twins, mmi_cdiv(G * NC + G * Dh + G, 128), 128, 0, s, t, tokens, masked_until, no_text, offsets_m, rope, Dh);
            if (temb2) MMI_LAUNCH(k_lm_embed_demux, dim3(mmi_cdiv(d, 256), B), 256, 0, s, (const int*)tokens, NC, emb, card1, temb, temb2,
                                  text_n, x, d, T, xks, cond);
            else MMI_LAUNCH(k_lm_embed, dim3(mmi_cdiv(d, 256), B), 256, 0, s, (const int*)tokens, NC, emb, card1, temb, x, d, T, xks, cond);
            MMI_CHECK_LAUNCH();
            return (int)MMI_OK;
        });
    }
    // ---- temporal transformer
    const int NS = attn_splits(lm->knobs, c, B);
    lm->attn_ns = NS;
    const int kvf = lm->ring.form;
    const size_t kv_layer = lm->ring.layer_u16;  // in uint16 units: an fp8 ring is half as large
    Pending pending;   // split-K partials of the previous linear_out still to be folded into x
    // the int8 linears that read the normalised rows (in_proj, ffn_in) take their int8 copy
    const void* xn_in = a8 ? (const void*)lm->xnq : lm->xn;
    const Q8 xn_q8 = a8 ? Q8{3, lm->sx_xn} : Q8{};
    for (int l = 0; l < c.num_layers; ++l) {
        const LayerW& L = lm->layers[l];
        P.site("L.norm1");
        add_resid_rmsnorm(lm, lm->x, pending, L.n1, lm->xn, d, a8 ? lm->xnq : nullptr, a8 ? lm->sx_xn : nullptr);
        if (l == 1) add_hidden_tap(lm, 0);     // x is complete (the previous linear_out's partials folded in) right after this norm
        LmAttnArgs a;
        a.qrot = lm->qrot; a.kc = lm->kc + l * kv_layer; a.vc = lm->vc + l * kv_layer;
        a.offsets = lm->offsets_m; a.opart = lm->opart; a.ml = lm->ml; a.out = lm->att;
        a.B = B; a.H = H; a.Dh = Dh; a.cap = c.context; a.context = c.context; a.NS = NS; a.max_period = c.max_period;
        a.T = lm->T; a.out_ksteps = packed_ksteps(lm, d);
        a.done = lm->attn_done; a.solo_rows = attn_solo_rows(lm->knobs, B * H);
        a.kv_soff = (long)lm->ring.scale_off;
        P.site("L.in_proj");
        {   // in_proj with RoPE + ring-KV write in its epilogue
            GemmOpt o;
            o.ring = &a;
            o.q8 = xn_q8;
            add_gemm(lm, L.in_proj, xn_in, MMI_EPI_ROPE_KV, {}, o);
        }
        P.site("L.attn");
        const bool wave = attn_wave_kernel(lm->knobs);
        P.add([=](hipStream_t s) { return launch_attn(s, a, kvf, wave, a.NS > 1 && (!wave || lm->prog.variant == 1)); });
        P.site("L.out_proj");
        if (a8) {
            add_quant_rows(lm, lm->att, lm->attq, lm->sx_att, d);
            pending = add_gemm_resid(lm, L.out_proj, lm->attq, lm->x, d, Q8{3, lm->sx_att});
        } else
        pending = add_gemm_resid(lm, L.out_proj, lm->att, lm->x, d);
        if (c.cross_attention) {   // x = x + cross_attention(norm_cross(x), src, src) (transformer.py:779-786)
            P.site("L.norm_cross");
            {
                const int T = lm->T, ksteps = packed_ksteps(lm, d), Pn = pending.P;
                uint16_t *x = lm->x, *y = lm->xn; const float* partial = lm->partial;
                const uint16_t *w = L.nx_w, *bb = L.nx_b;
                P.add([=](hipStream_t s) {
                    MMI_LAUNCH(k_resid_layernorm, B, row_threads(d), 0, s, x, partial, Pn, B, w, bb, y, d, T, ksteps, 1e-5f);
                    MMI_CHECK_LAUNCH();
                    return (int)MMI_OK;
                });
            }
            P.site("L.cross_q");
            add_gemm(lm, L.x_q, lm->xn, MMI_EPI_STORE, {lm->qrot, d});
            P.site("L.cross_attn");
            {
                CrossAttnArgs ca;
                ca.q = lm->qrot; ca.kv = lm->xkv + (size_t)l * B * lm->cross_cap * 2 * d; ca.out = lm->att;
                ca.len = lm->xlen; ca.B = B; ca.H = H; ca.Dh = Dh; ca.cap = lm->cross_cap; ca.T = lm->T; ca.out_ksteps = packed_ksteps(lm, d);
                P.add([=](hipStream_t s) { return launch_cross_attn(s, ca); });
            }
            P.site("L.cross_out");
            pending = add_gemm_resid(lm, L.x_out, lm->att, lm->x, d);
        }
        P.site("L.norm2");
        add_resid_rmsnorm(lm, lm->x, pending, L.n2, lm->xn, d, a8 ? lm->xnq : nullptr, a8 ? lm->sx_xn : nullptr);
        P.site("L.ffn_in");
        {
            GemmOpt o;
            o.dominant = true;
            o.q8 = xn_q8;
            add_gemm(lm, L.ffn_in, xn_in, MMI_EPI_GATE, {lm->hb, c.ffn_hidden, true}, o);
        }
        P.site("L.ffn_out");
        if (a8) {
            add_quant_rows(lm, lm->hb, lm->hbq, lm->sx_hb, c.ffn_hidden);
            pending = add_gemm_resid(lm, L.ffn_out, lm->hbq, lm->x, d, Q8{3, lm->sx_hb});
        } else
        pending = add_gemm_resid(lm, L.ffn_out, lm->hb, lm->x, d);
    }
    P.site("out_norm");
    add_resid_rmsnorm(lm, lm->x, pending, lm->out_norm, lm->tout, d, a8 ? lm->toutq : nullptr, a8 ? lm->sx_tout : nullptr);
    if (c.num_layers == 1) add_hidden_tap(lm, 0);
    add_hidden_tap(lm, 1);
    // the int8 linears that read transformer_out (text head, depformer_in) take its int8 copy
    const void* tout_in = a8 ? (const void*)lm->toutq : lm->tout;
    GemmOpt from_tout;
    if (a8) from_tout.q8 = Q8{3, lm->sx_tout};
    P.site("text_linear");
    add_gemm(lm, lm->text_linear, tout_in, MMI_EPI_STORE, {lm->text_logits, c.text_card_out}, from_tout);
    // depformer_in[k](transformer_out) for every micro-step in one launch; each sampler then adds its token's embedding row
    // and writes the next micro-step's input (lm.py:465-470) - 8 dependent launches less on the sequential chain
    const bool grouped = lm->dep_in_grouped && !lm->lora_on;     // (an adapter handle: one depformer_in, one bank, per micro-step)
    lm->op_depformer = P.ops.size();
    P.site("dep.in_all");
    if (grouped) add_gemm(lm, lm->dep_in_all, tout_in, MMI_EPI_STORE, {lm->dpre, lm->dep_nw * dd}, from_tout);
    P.site("text_sample");
    // a demuxed text stream: the first input row is written by its own launch behind the sampler (and behind an on_text_hook,
    // which may mux a second token into the one sampled)
    // the TTS machine writes that row itself, from ITS token: the sampler's fused write is off, and on a demuxed model the
    // machine's launch stands where dep.in_demux stood
    add_sample(lm, lm->text_logits, c.text_card_out, c.text_card_out, true, 0, lm->text_tok, 1, grouped && !lm->demux && !lm->tts ? 0 : -1);
    if (lm->tts) {
        P.site("tts.machine");
        SampleArgs na;
        memset(&na, 0, sizeof(na));
        if (grouped) {
            na.nx_pre = lm->dpre + (size_t)lm->dep_sched[0] * dd; na.nx_ld = lm->dep_nw * dd;
            na.nx_emb = lm->dep_emb[0]; na.nx_out = lm->dx;
            na.nx_D = dd; na.nx_T = lm->Td; na.nx_ksteps = packed_ksteps_t(lm, lm->Td, dd);
        }
        na.nx_dup = lm->cfg_coef != 1.f ? lm->gen_batch : 0;
        na.out_stride = 1;
        TtsArgs m;
        memset(&m, 0, sizeof(m));
        m.st = lm->tts; m.stride = lm->tts_stride; m.max_entries = lm->tts_max_entries; m.max_tokens = lm->tts_max_tokens;
        m.max_prefix = lm->tts_max_prefix; m.p = lm->tts_p; m.offsets = lm->offsets; m.exec = lm->exec; m.text_tok = lm->text_tok;
        m.emb2 = lm->demux ? lm->dep_emb2 : nullptr; m.demux_n = c.text_card + 1;
        const int G = lm->gen_batch;
        P.add([=](hipStream_t s) {
            MMI_LAUNCH(k_tts_machine, G, 128, 0, s, na, m);
            MMI_CHECK_LAUNCH();
            return (int)MMI_OK;
        });
        // an on_text_hook next to the machine runs behind it and sees its token; the row is then rebuilt from what the hook left
        lm->op_after_text_sample = P.ops.size();
        lm->text_sample_args = na;
    } else if (lm->demux && c.dep_q > 0) {
        P.site("dep.in_demux");
        SampleArgs na;
        memset(&na, 0, sizeof(na));
        na.nx_pre = lm->dpre + (size_t)lm->dep_sched[0] * dd; na.nx_ld = lm->dep_nw * dd;
        na.nx_emb = lm->dep_emb[0]; na.nx_out = lm->dx;
        na.nx_D = dd; na.nx_T = lm->Td; na.nx_ksteps = packed_ksteps_t(lm, lm->Td, dd);
        na.nx_dup = lm->cfg_coef != 1.f ? lm->gen_batch : 0;
        na.out_stride = 1;
        const int G = lm->gen_batch, N = c.text_card + 1;
        const int* tt = lm->text_tok; const uint16_t* e2 = lm->dep_emb2;
        P.add([=](hipStream_t s) {
            MMI_LAUNCH(k_dep_next_input_demux, G, 128, 0, s, na, tt, e2, N);
            MMI_CHECK_LAUNCH();
            return (int)MMI_OK;
        });
    }
    // ---- depformer: dep_q sequential micro-steps
    const size_t dkv_layer = (size_t)B * Hd * c.dep_q * Dhd;
    const GemmOut dx_out{lm->dx, dd, true};       // out_proj and linear_out: dx += linear(.), in place
    GemmOpt onto_dx;
    onto_dx.resid = lm->dx;
    for (int k = 0; k < c.dep_q; ++k) {
        const int* prev = k == 0 ? lm->text_tok : lm->audio_tok + (k - 1);
        const int prev_stride = k == 0 ? 1 : c.dep_q;
        P.site("dep.in");
        if (!grouped) {
            GemmOpt o = from_tout;
            o.emb = lm->dep_emb[k]; o.tok = prev; o.tok_stride = prev_stride;
            add_gemm(lm, lm->dep_in[k], tout_in, MMI_EPI_EMB, {lm->dx, dd, true}, o);
        }
        for (int l = 0; l < c.depformer_num_layers; ++l) {
            const DepLayerW& L = lm->dep_layers[l];
            P.site("dep.in_proj");
            // micro-step 0 attends to one position: softmax over one score is 1 and the attention output is v itself, so in_proj's
            // epilogue writes k / v into the frame's cache and v as out_proj's operand, and the attention launch is dropped
            // (bit-identical: 1 * v / 1; knobs.dep_attn0_launch keeps the launch)
            const bool skip_attn0 = k == 0 && Dhd % 8 == 0 && !lm->knobs.dep_attn0_launch;
            if (skip_attn0) {
                const DepKv kv{lm->dkc + l * dkv_layer, lm->dvc + l * dkv_layer, Hd, Dhd, c.dep_q};
                add_norm_gemm(lm, L.in_proj[k], lm->dx, L.n1, lm->dxn, dd, MMI_EPI_DEP_QKV0, {lm->datt, dd, true}, kv);
            } else
            add_norm_gemm(lm, L.in_proj[k], lm->dx, L.n1, lm->dxn, dd, MMI_EPI_STORE, {lm->dqkv, 3 * dd});
            DepAttnArgs da;
            da.qkv = lm->dqkv; da.kc = lm->dkc + l * dkv_layer; da.vc = lm->dvc + l * dkv_layer; da.out = lm->datt;
            da.B = B; da.H = Hd; da.Dh = Dhd; da.steps = c.dep_q; da.k = k;
            da.T = lm->Td; da.out_ksteps = packed_ksteps_t(lm, lm->Td, dd);
            P.site("dep.attn");
            const bool attn_in_gemm = !skip_attn0 && dep_attn_fusable(lm, L.out_proj[k], Hd, Dhd, c.dep_q, lm->batch);
            if (!skip_attn0 && !attn_in_gemm)
            P.add([=](hipStream_t s) { return launch_dep_attn(s, da); });
            // int8 activations: the chain's linears quantise their own input row inside the GEMM (k_gemm_q8)
            P.site("dep.out_proj");
            if (attn_in_gemm) add_dep_attn_out_proj(lm, L.out_proj[k], da, lm->dx, dd);
            else if (a8) add_q8_gemm(lm, L.out_proj[k], lm->datt, dd, MMI_EPI_RESID, dx_out, lm->dx);
            else add_gemm(lm, L.out_proj[k], lm->datt, MMI_EPI_RESID, dx_out, onto_dx);
            P.site("dep.ffn_in");
            add_norm_gemm(lm, L.ffn_in[k], lm->dx, L.n2, lm->dxn, dd, MMI_EPI_GATE, {lm->dhb, c.depformer_ffn_hidden, true});
            P.site("dep.ffn_out");
            if (a8) add_q8_gemm(lm, L.ffn_out[k], lm->dhb, c.depformer_ffn_hidden, MMI_EPI_RESID, dx_out, lm->dx);
            else add_gemm(lm, L.ffn_out[k], lm->dhb, MMI_EPI_RESID, dx_out, onto_dx);
        }
        uint16_t* lg = lm->dlogits + (size_t)k * B * c.card;
        P.site("dep.lin");
        if (a8) add_q8_gemm(lm, lm->dep_lin[k], lm->dx, dd, MMI_EPI_STORE, {lg, c.card});
        else add_gemm(lm, lm->dep_lin[k], lm->dx, MMI_EPI_STORE, {lg, c.card});
        P.site("dep.sample");
        add_sample(lm, lg, c.card, c.card, false, 1 + k, lm->audio_tok + k, c.dep_q, grouped && k + 1 < c.dep_q ? k + 1 : -1);
    }
    // ---- token ring out
    // log-probabilities of the tokens the commit is about to store (an enabled handle): one launch, and the hooked step's cut in
    // front of it, so that it sees the tokens on_text_token / on_audio_tokens left
    lm->op_commit = P.ops.size();
    if (lm->lp.lp) {
        P.site("logprob");
        const LpArgs la = step_logprob_args(lm);
        P.add([=](hipStream_t s) { return launch_step_logprob(s, la, la.t.B); });
    }
    P.site("commit");
    {
        TokArgs t = tok_args(lm);
        const int *tt = lm->text_tok, *at = lm->audio_tok; int* out = lm->out_i32; unsigned long long* rng = lm->rng;
        P.add([=](hipStream_t s) {
            TokArgs tc = t;
            if (lm->tts_rule_done) tc.tts_audio = 0;      // a hooked step: k_tts_audio_rule ran in front of on_audio_tokens
            MMI_LAUNCH(k_lm_commit, mmi_cdiv(tc.B, 64), 64, 0, s, tc, tt, at, out, rng);
            MMI_CHECK_LAUNCH();
            return (int)MMI_OK;
        });
    }
    return MMI_OK;
}

// keys | values of the cross-attention source for every temporal layer (transformer.py:495-505: `linear(src, in_proj.weight[dim:])`,
// bf16): the `ncol` source positions src [ncol][dim] land in slots [slot0, slot0 + ncol) of every layer's [batch * cross_cap]
// slots, through the weight-streaming GEMM as batches of T "sessions".  At streaming_start with cap == cross_len that is every
// row at once; otherwise, and for mmi_lm_set_row_condition, one model row's positions into that row's slots.  A position's
// keys / values do not depend on its column in the tile nor on the tile's fill (every launch has mt = 1), so both give the same bits.
int project_cross_source(mmi_lm* lm, const uint16_t* src, size_t slot0, int ncol, hipStream_t s) {
    const mmi_lm_cfg& c = lm->cfg;
    const int d = c.dim, T = lm->T, ksteps = packed_ksteps(lm, d);
    const size_t slots = (size_t)lm->batch * lm->cross_cap;
    uint16_t* xp = lm->xn;                                        // packed scratch of >= one batch tile
    for (int col0 = 0; col0 < ncol; col0 += T) {
        const int n = ncol - col0 < T ? ncol - col0 : T;
        MMI_HIP_CHECK(hipMemsetAsync(xp, 0, (size_t)ksteps * 512 * sizeof(uint16_t), s));
        MMI_LAUNCH(k_pack_rows, mmi_cdiv(n * d, 256), 256, 0, s, src + (size_t)col0 * d, n, d, xp, T, ksteps);
        MMI_CHECK_LAUNCH();
        for (int l = 0; l < c.num_layers; ++l) {
            const GemmArgs a = gemm_args(lm, T, xp, MMI_EPI_STORE, n, n, {lm->xkv + ((size_t)l * slots + slot0 + col0) * 2 * d, 2 * d});
            int rc = launch_gemm(lm, s, lm->layers[l].x_kv, a, false);
            if (rc) return rc;
        }
    }
    // the packed scratch goes back to all-zero padding (the step's producers only write the live rows)
    MMI_HIP_CHECK(hipMemsetAsync(xp, 0, packed_elems(lm, d) * sizeof(uint16_t), s));
    return MMI_OK;
}

int check_cfg(const mmi_lm_cfg& c) {
    if (c.dim % c.num_heads || c.depformer_dim % c.depformer_num_heads) return mmi_fail(MMI_ERR_UNSUPPORTED, "dim % heads != 0");
    const int Dh = c.dim / c.num_heads, Dhd = c.depformer_dim / c.depformer_num_heads;
    if (c.kv_cache_dtype == MMI_F4E2M1X2 && Dh % 32)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "4-bit KV needs a head dim multiple of 32 (a 16-byte load of the ring is two blocks of 16)");
    if (Dh != 32 && Dh != 64 && Dh != 128) return mmi_fail(MMI_ERR_UNSUPPORTED, "temporal head dim must be 32/64/128");
    if (Dhd > 64 || Dhd < 1) return mmi_fail(MMI_ERR_UNSUPPORTED, "depformer head dim must be <= 64");
    if (c.kv_cache_dtype != 0 && c.kv_cache_dtype != MMI_BF16 && c.kv_cache_dtype != MMI_F8E4M3 && c.kv_cache_dtype != MMI_F4E2M1X2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "kv_cache_dtype must be MMI_BF16, MMI_F8E4M3 or MMI_F4E2M1X2");
    if (c.kv_cache_dtype == MMI_F8E4M3 && (c.dim / c.num_heads) % 16) return mmi_fail(MMI_ERR_UNSUPPORTED, "fp8 KV needs a head dim multiple of 16");
    if (c.card % 8 || c.text_card_out % 8 || c.card > 32768 || c.text_card_out > 32768)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "vocabulary sizes must be multiples of 8 and at most 32768");
    if (c.dep_q < 0 || c.dep_q > 32 || c.n_q < c.dep_q || c.n_q + 1 > 64) return mmi_fail(MMI_ERR_UNSUPPORTED, "bad n_q / dep_q");
    if (c.dim > 8 * 1024 * MMI_NORM_MAXP || c.depformer_dim > 8 * 1024 * MMI_NORM_MAXP)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "model width above the RMSNorm kernel's register budget");
    if (c.dim % 8 || c.depformer_dim % 8 || c.ffn_hidden % 8 || c.depformer_ffn_hidden % 8)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "feature sizes must be multiples of 8");
    return MMI_OK;
}

// LMGen's per-step hooks (lm.py:734-757): the launch list cut at the text sampler and at the ring commit, run eagerly, with
// the host callbacks in between.  Nothing synchronises: the hooks enqueue their copies / kernels on the same stream.
int run_step_with_hooks(mmi_lm* lm, hipStream_t s) {
    MmiProgram& P = lm->prog;
    auto call = [&](int (*fn)(void*)) -> int {
        if (!fn) return MMI_OK;
        lm->in_hook = true;
        const int r = fn(lm->hooks.user);
        lm->in_hook = false;
        return r ? mmi_fail(MMI_ERR_INVALID, "a step hook reported an error") : MMI_OK;
    };
    int rc;
    if (lm->phase_fn && lm->op_depformer <= lm->op_text_sample) {       // mmi_lm_set_phase_callback: the same point as in the un-hooked step
        if ((rc = P.run_range(s, 0, lm->op_depformer))) return rc;
        if (lm->phase_fn(lm->phase_user, (mmi_stream)s)) return mmi_fail(MMI_ERR_INVALID, "the phase callback reported an error");
        rc = P.run_range(s, lm->op_depformer, lm->op_text_sample);
    } else rc = P.run_range(s, 0, lm->op_text_sample);
    if (rc || (rc = call(lm->hooks.on_text_logits))) return rc;
    if ((rc = P.run_range(s, lm->op_text_sample, lm->op_after_text_sample))) return rc;
    if (lm->hooks.on_text_token) {
        if ((rc = call(lm->hooks.on_text_token))) return rc;
        // the sampler also wrote the depth transformer's first input row from ITS token (fused, lm.py:465-470): redo that
        // row from the token the hook left behind
        if (lm->text_sample_args.nx_out) {
            if (lm->tts && lm->demux)
                MMI_LAUNCH(k_dep_next_input_demux, lm->gen_batch, 128, 0, s, lm->text_sample_args, (const int*)lm->text_tok,
                           (const uint16_t*)lm->dep_emb2, lm->cfg.text_card + 1);
            else
            MMI_LAUNCH(k_dep_next_input, lm->gen_batch, 128, 0, s, lm->text_sample_args, (const int*)lm->text_tok);
            MMI_CHECK_LAUNCH();
        }
    }
    if ((rc = P.run_range(s, lm->op_after_text_sample, lm->op_commit))) return rc;
    if (lm->cfg.dep_q > 0 && lm->hooks.on_audio_tokens) {      // no depformer, no audio tokens (lm.py:748-749)
        if (lm->tts) {          // the machine's audio rule first: the hook sees its tokens, the commit stores what the hook leaves
            TokArgs t = tok_args(lm);
            MMI_LAUNCH(k_tts_audio_rule, mmi_cdiv(t.B * t.dep_q, 64), 64, 0, s, t, lm->audio_tok);
            MMI_CHECK_LAUNCH();
            lm->tts_rule_done = true;
        }
        if ((rc = call(lm->hooks.on_audio_tokens))) { lm->tts_rule_done = false; return rc; }
    }
    rc = P.run_range(s, lm->op_commit, P.ops.size());
    lm->tts_rule_done = false;
    return rc;
}

}  // namespace

// ===============================================================================================
// C ABI
// ===============================================================================================
extern "C" int mmi_lm_create(const mmi_lm_cfg* cfg, const mmi_tensor_desc* weights, int32_t n_weights, int32_t max_batch,
                             mmi_lm** out) {
    return mmi_lm_create_ext(cfg, nullptr, weights, n_weights, max_batch, out);
}

static int lm_create_rows(const mmi_lm_cfg* cfg, const mmi_lm_cfg_ext* ext, const mmi_tensor_desc* weights, int32_t n_weights,
                          int32_t max_batch, mmi_lm** out);

// MXFP4 linears (`weight` MMI_F4E2M1X2 + `weight_scale_e8m0` MMI_E8M0): everything that can be refused is refused here, from the
// descriptors and the scale bytes, before anything is allocated or packed.  The scale range 2..252 keeps every dequantised weight
// a normal, finite bf16 (0.5 * 2^(2-127) = 2^-126 is the smallest normal; 6 * 2^(253-127) would overflow), which is what makes the
// conversion exact (mmi_fp4.h).
static int check_mxfp4_descs(const mmi_lm_cfg& c, bool low_rank_or_demux, const mmi_tensor_desc* weights, int32_t n_weights) {
    MmiWeights W{weights, n_weights};
    bool any = false;
    for (int i = 0; i < n_weights; ++i) any = any || weights[i].dtype == MMI_F4E2M1X2;
    if (!any) return MMI_OK;
    if (c.cross_attention) return mmi_fail(MMI_ERR_UNSUPPORTED, "cross-attention layers with quantised linears are not supported");
    if (low_rank_or_demux) return mmi_fail(MMI_ERR_UNSUPPORTED, "quantised linears with low-rank or demuxed embeddings are not supported");
    std::vector<uint8_t> host;
    for (int i = 0; i < n_weights; ++i) {
        const mmi_tensor_desc& d = weights[i];
        const std::string name = d.name ? d.name : "";
        if (d.dtype == MMI_I8 || d.dtype == MMI_F8E4M3) return mmi_fail(MMI_ERR_UNSUPPORTED, "mixed bf16 / int8 / fp8 linear weights: " + name);
        if (d.dtype != MMI_F4E2M1X2) continue;
        if (d.ndim != 2) return mmi_fail(MMI_ERR_SHAPE, "unexpected rank for " + name);
        const int64_t N = d.shape[0], K = 2 * d.shape[1];
        if (K % 32 != 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "MXFP4 linears need in_features to be a multiple of 32: " + name);
        const std::string sname = name + "_scale_e8m0";
        const mmi_tensor_desc* sc = W.find(sname);
        if (!sc) return mmi_fail(MMI_ERR_MISSING_WEIGHT, "missing weight: " + sname);
        if (sc->dtype != MMI_E8M0 || sc->ndim != 2 || sc->shape[0] != N || sc->shape[1] != K / 32)
            return mmi_fail(MMI_ERR_SHAPE, "MXFP4 block scales must be e8m0 [out_features, in_features / 32]: " + sname);
        host.resize((size_t)(N * (K / 32)));
        if (host.empty()) continue;
        MMI_HIP_CHECK(hipMemcpy(host.data(), sc->data, host.size(), hipMemcpyDeviceToHost));
        for (uint8_t b : host) {
            if (b == 255) return mmi_fail(MMI_ERR_INVALID, "MXFP4 block scale 255 is the E8M0 NaN: " + sname);
            if (b < 2 || b > 252)
                return mmi_fail(MMI_ERR_UNSUPPORTED, "MXFP4 block scales must be 2..252 (2^-125..2^125: every weight a normal, finite bf16), found " +
                                                         std::to_string((int)b) + ": " + sname);
        }
    }
    return MMI_OK;
}

extern "C" int mmi_lm_create_ext(const mmi_lm_cfg* cfg, const mmi_lm_cfg_ext* ext, const mmi_tensor_desc* weights, int32_t n_weights,
                                 int32_t max_batch, mmi_lm** out) {
    if (max_batch > 64)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "max_batch > 64 sessions per GPU is not supported by mmi_lm_create / mmi_lm_create_ext: "
                                             "mmi_lm_create_rows takes up to 128 model rows (bf16 linears)");
    return lm_create_rows(cfg, ext, weights, n_weights, max_batch, out);
}

// Up to 128 model rows per handle: above 64 the step's linears run on k_gemm_rows (3 or 4 batch tiles of 32, bf16 weights).
// max_rows <= 64 is mmi_lm_create_ext: the same launch lists, the same bits.
extern "C" int mmi_lm_create_rows(const mmi_lm_cfg* cfg, const mmi_lm_cfg_ext* ext, const mmi_tensor_desc* weights, int32_t n_weights,
                                  int32_t max_rows, mmi_lm** out) {
    if (max_rows > 128) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_create_rows: max_rows > 128 model rows per handle is not supported");
    return lm_create_rows(cfg, ext, weights, n_weights, max_rows, out);
}

static int lm_create_rows(const mmi_lm_cfg* cfg, const mmi_lm_cfg_ext* ext, const mmi_tensor_desc* weights, int32_t n_weights,
                          int32_t max_batch, mmi_lm** out) {
    const MmiKnobs knobs = mmi_knobs_from_env();     // the handle's one reading of the environment
    if (!cfg || !weights || !out || max_batch <= 0) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_create: bad argument");
    mmi_lm_cfg norm_cfg = *cfg;
    if (norm_cfg.dep_q == 0) {   // "No-Depformer --- e.g., an ASR model" (lm.py:218-221): text stream only; the depth-transformer
        norm_cfg.depformer_num_layers = 0;   // fields are then unused, give them inert values so that the sizing code stays generic
        norm_cfg.depformer_dim = 8; norm_cfg.depformer_num_heads = 1; norm_cfg.depformer_ffn_hidden = 8;
    }
    int rc = check_cfg(norm_cfg);
    if (rc) return rc;
    mmi_lm_cfg_ext x;
    memset(&x, 0, sizeof(x));
    if (ext) x = *ext;
    // depformer weight schedule (lm.py:125-127, transformer.py:395-401): dep_q entries 0..max without gaps
    std::vector<int> sched(norm_cfg.dep_q);
    int nw = norm_cfg.dep_q;
    for (int k = 0; k < norm_cfg.dep_q; ++k) sched[k] = k;
    if (x.depformer_schedule_len) {
        if (x.depformer_schedule_len != norm_cfg.dep_q || norm_cfg.dep_q == 0)
            return mmi_fail(MMI_ERR_INVALID, "depformer_weights_per_step_schedule must have dep_q entries");
        nw = 0;
        for (int k = 0; k < norm_cfg.dep_q; ++k) {
            sched[k] = x.depformer_schedule[k];
            if (sched[k] < 0 || sched[k] >= norm_cfg.dep_q) return mmi_fail(MMI_ERR_INVALID, "depformer schedule entries must be in [0, dep_q)");
            nw = sched[k] + 1 > nw ? sched[k] + 1 : nw;
        }
        std::vector<char> seen(nw, 0);
        for (int k = 0; k < norm_cfg.dep_q; ++k) seen[sched[k]] = 1;
        for (int w = 0; w < nw; ++w)
            if (!seen[w]) return mmi_fail(MMI_ERR_INVALID, "depformer schedule must use every weight index 0..max (no gaps)");
    }
    const int low_rank = x.depformer_low_rank;
    if (low_rank < 0 || low_rank % 8) return mmi_fail(MMI_ERR_INVALID, "depformer_low_rank_embeddings must be a multiple of 8");
    const bool demux = x.demux_second_text_stream != 0;
    if (max_batch > 64)   // k_gemm_rows is bf16.  Mixed widths are refused by load_linear, so any quantised linear's descriptor
        for (int i = 0; i < n_weights; ++i)   // settles it - before a byte of the model is uploaded and packed
            if (weights[i].ndim == 2 && (weights[i].dtype == MMI_I8 || weights[i].dtype == MMI_F8E4M3))
                return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_create_rows: int8 / fp8 linears are not supported above 64 model rows (k_gemm_rows is bf16)");
    if (max_batch > 64)
        for (int i = 0; i < n_weights; ++i)
            if (weights[i].dtype == MMI_F4E2M1X2)
                return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_create_rows: MXFP4 linears are not supported above 64 model rows (k_gemm_rows is bf16)");
    if ((rc = check_mxfp4_descs(norm_cfg, low_rank != 0 || demux, weights, n_weights))) return rc;
    mmi_lm* lm = new mmi_lm();
    lm->knobs = knobs;
    lm->wts.poison = lm->st.poison = knobs.debug_poison;
    lm->prog.skip = knobs.skip_sites;
    lm->dep_sched = sched;
    lm->dep_nw = nw;
    lm->demux = demux;
    lm->dep_low_rank = low_rank != 0;
    if (hipGetDevice(&lm->device) != hipSuccess) lm->device = -1;
    lm->cfg = norm_cfg;
    lm->max_batch = max_batch;
    lm->T = max_batch <= 16 ? 16 : 32;
    if (knobs.lm_tile == 32 || (knobs.lm_tile == 16 && max_batch <= 16)) lm->T = knobs.lm_tile;     // A/B hook: the 32-row tile at small batches
    lm->use_graph = !knobs.no_graph;
    const mmi_lm_cfg& c = lm->cfg;
    lm->NC = c.n_q + 1;
    lm->max_delay = 0;
    for (int i = 0; i < lm->NC; ++i) lm->max_delay = c.delays[i] > lm->max_delay ? c.delays[i] : lm->max_delay;
    lm->CT = lm->max_delay + 2;
    MmiWeights W{weights, n_weights};
    auto fail = [&](int code) { mmi_lm_destroy(lm); return code; };
    const int d = c.dim, dd = c.depformer_dim;
    // embeddings (lm.py:135-139, 189-196): row gathers, kept as stored
    {
        const size_t per = (size_t)(c.card + 1) * d;
        if (hipSuccess != lm->wts.alloc(&lm->emb, per * c.n_q)) return fail(mmi_fail(MMI_ERR_HIP, "out of device memory"));
        for (int i = 0; i < c.n_q; ++i)
            if ((rc = load_copy(lm, W, "emb." + std::to_string(i) + ".weight", 2, per, nullptr, lm->emb + per * i))) return fail(rc);
        const int N = c.text_card + 1;
        if (demux) {
            if ((rc = load_expanded(lm, W, "text_emb", N, d, d, ".out1.weight", &lm->text_emb))) return fail(rc);
            if ((rc = load_expanded(lm, W, "text_emb", N, d, d, ".out2.weight", &lm->text_emb2))) return fail(rc);
        } else if ((rc = load_copy(lm, W, "text_emb.weight", 2, (size_t)N * d, &lm->text_emb))) return fail(rc);
        lm->dep_emb.resize(c.dep_q);
        const int r = low_rank ? low_rank : dd;
        if (c.dep_q > 0) {
            // lm_utils.py:95-124: a demuxed table goes through out1 / out2 (its `low_rank` linear is not applied), a low-rank one
            // through `low_rank`
            if (demux) {
                if ((rc = load_expanded(lm, W, "depformer_text_emb", N, r, dd, ".out1.weight", &lm->dep_emb[0]))) return fail(rc);
                if ((rc = load_expanded(lm, W, "depformer_text_emb", N, r, dd, ".out2.weight", &lm->dep_emb2))) return fail(rc);
            } else if (low_rank) {
                if ((rc = load_expanded(lm, W, "depformer_text_emb", N, r, dd, ".low_rank.weight", &lm->dep_emb[0]))) return fail(rc);
            } else if ((rc = load_copy(lm, W, "depformer_text_emb.weight", 2, (size_t)N * dd, &lm->dep_emb[0]))) return fail(rc);
        }
        for (int k = 1; k < c.dep_q; ++k) {
            const std::string name = "depformer_emb." + std::to_string(k - 1);
            if (low_rank) rc = load_expanded(lm, W, name, c.card + 1, r, dd, ".low_rank.weight", &lm->dep_emb[k]);
            else rc = load_copy(lm, W, name + ".weight", 2, (size_t)(c.card + 1) * dd, &lm->dep_emb[k]);
            if (rc) return fail(rc);
        }
    }
    // temporal transformer (lm.py:146-158)
    lm->layers.resize(c.num_layers);
    for (int l = 0; l < c.num_layers; ++l) {
        LayerW& L = lm->layers[l];
        std::string p = "transformer.layers." + std::to_string(l);
        if ((rc = load_linear(lm, W, p + ".self_attn.in_projs.0.weight", 3 * d, d, 0, &L.in_proj))) return fail(rc);
        if ((rc = load_linear(lm, W, p + ".self_attn.out_projs.0.weight", d, d, 0, &L.out_proj))) return fail(rc);
        if ((rc = load_linear(lm, W, p + ".gating.linear_in.weight", 2 * c.ffn_hidden, d, c.ffn_hidden, &L.ffn_in))) return fail(rc);
        if ((rc = load_linear(lm, W, p + ".gating.linear_out.weight", d, c.ffn_hidden, 0, &L.ffn_out))) return fail(rc);
        if ((rc = load_copy(lm, W, p + ".norm1.alpha", 3, d, &L.n1))) return fail(rc);
        if ((rc = load_copy(lm, W, p + ".norm2.alpha", 3, d, &L.n2))) return fail(rc);
        if (c.cross_attention) {
            if (d % lm->T) return fail(mmi_fail(MMI_ERR_UNSUPPORTED, "cross-attention needs dim to be a multiple of the GEMM tile"));
            if ((rc = load_linear(lm, W, p + ".cross_attention.in_projs.0.weight", 3 * d, d, 0, &L.x_in))) return fail(rc);
            if ((rc = load_linear(lm, W, p + ".cross_attention.out_projs.0.weight", d, d, 0, &L.x_out))) return fail(rc);
            if (L.x_in.wq) return fail(mmi_fail(MMI_ERR_UNSUPPORTED, "cross-attention layers with quantised linears are not supported"));
            if ((rc = load_copy(lm, W, p + ".norm_cross.weight", 1, d, &L.nx_w))) return fail(rc);
            if ((rc = load_copy(lm, W, p + ".norm_cross.bias", 1, d, &L.nx_b))) return fail(rc);
            const int ntq = d / lm->T;                               // n-tiles of the query rows; the rest are keys | values
            L.x_q = L.x_in;  L.x_q.N = d;      L.x_q.NT = ntq;
            L.x_kv = L.x_in; L.x_kv.N = 2 * d; L.x_kv.NT = 2 * ntq;
            L.x_kv.wp = L.x_in.wp + (size_t)ntq * L.x_in.KSTEPS * 64;
            L.x_q.bytes = L.x_in.bytes / 3; L.x_kv.bytes = L.x_in.bytes - L.x_q.bytes;
        }
    }
    if ((rc = load_copy(lm, W, "out_norm.alpha", 3, d, &lm->out_norm))) return fail(rc);
    if ((rc = load_linear(lm, W, "text_linear.weight", c.text_card_out, d, 0, &lm->text_linear))) return fail(rc);
    if (c.extra_heads_num_heads > 0) {   // lm.py:224-226: nn.Linear(dim, extra_heads_dim, bias=False) read by step_with_extra_heads
        if (c.extra_heads_dim < 1 || c.extra_heads_dim > 64) return fail(mmi_fail(MMI_ERR_UNSUPPORTED, "extra_heads_dim must be 1..64"));
        const size_t per = (size_t)c.extra_heads_dim * d;
        if (hipSuccess != lm->wts.alloc(&lm->extra_heads_all, per * c.extra_heads_num_heads)) return fail(mmi_fail(MMI_ERR_HIP, "out of device memory"));
        for (int i = 0; i < c.extra_heads_num_heads; ++i)
            if ((rc = load_copy(lm, W, "extra_heads." + std::to_string(i) + ".weight", 2, per, nullptr, lm->extra_heads_all + per * i))) return fail(rc);
    }
    // depformer (lm.py:179-232; per-step weights transformer.py:291-318)
    lm->dep_in.resize(nw);
    lm->dep_lin.resize(c.dep_q);
    {
        // depformer_in[k] all read transformer_out, so they are packed back to back and run as ONE GEMM with
        // dep_q * depformer_dim output features ahead of the micro-step loop (build_program).  Needs whole n-tiles per step.
        const bool group = c.dep_q > 0 && dd % lm->T == 0 && !knobs.no_dep_in_group;
        uint8_t *wp_all = nullptr, *s4_all = nullptr;
        float *scale_all = nullptr, *scb_all = nullptr;
        size_t per = 0, per4 = 0;
        if (group) {
            const int NT = dd / lm->T, ksteps = mmi_cdiv(d, mmi_kstep(lm->T));
            per = lm->q8 == 4 ? (size_t)NT * mmi_cdiv(ksteps, 4) * 1024
                  : lm->q8 >= 1 ? (size_t)NT * mmi_cdiv(ksteps, 2) * 1024 : (size_t)NT * ksteps * 512 * sizeof(uint16_t);
            per4 = lm->q8 == 4 ? (size_t)NT * mmi_cdiv(ksteps, 4) * 64 * (lm->T == 32 ? 2 : 4) : 0;
            if (lm->wts.alloc(&wp_all, per * nw) != hipSuccess) return fail(mmi_fail(MMI_ERR_HIP, "out of device memory (depformer_in)"));
            if (per4 && lm->wts.alloc(&s4_all, per4 * nw) != hipSuccess)
                return fail(mmi_fail(MMI_ERR_HIP, "out of device memory (depformer_in scales)"));
            if (lm->q8 >= 1 && lm->q8 != 4 && lm->wts.alloc(&scale_all, (size_t)dd * nw) != hipSuccess)
                return fail(mmi_fail(MMI_ERR_HIP, "out of device memory (depformer_in scales)"));
            if (lm->q8 == 1 && lm->wts.alloc(&scb_all, (size_t)dd * nw) != hipSuccess)
                return fail(mmi_fail(MMI_ERR_HIP, "out of device memory (depformer_in scales)"));
        }
        for (int k = 0; k < nw; ++k) {
            if ((rc = load_linear(lm, W, "depformer_in." + std::to_string(k) + ".weight", dd, d, 0, &lm->dep_in[k],
                                  group ? wp_all + per * k : nullptr, scale_all ? scale_all + (size_t)dd * k : nullptr,
                                  scb_all ? scb_all + (size_t)dd * k : nullptr, 0, s4_all ? s4_all + per4 * k : nullptr)))
                return fail(rc);
        }
        for (int k = 1; group && k < nw; ++k)
            if (lm->dep_in[k].xinv != lm->dep_in[0].xinv)
                return fail(mmi_fail(MMI_ERR_UNSUPPORTED, "the depformer_in linears read the same tensor and must share one input_scale"));
        if (group) {
            lm->dep_in_all = lm->dep_in[0];
            lm->dep_in_all.N = dd * nw;
            lm->dep_in_all.NT = lm->dep_in[0].NT * nw;
            lm->dep_in_all.bytes = lm->dep_in[0].bytes * nw;
            lm->dep_in_grouped = true;
        }
        if (demux && c.dep_q > 0 && !group)
            return fail(mmi_fail(MMI_ERR_UNSUPPORTED, "a demuxed text stream needs depformer_dim to be a multiple of the GEMM tile"));
        // micro-step k reads weight set sched[k]: the per-step lists alias the nw packed sets (transformer.py:291-318)
        std::vector<GemmW> per_set = lm->dep_in;
        lm->dep_in.resize(c.dep_q);
        for (int k = 0; k < c.dep_q; ++k) lm->dep_in[k] = per_set[sched[k]];
    }
    // the depth transformer's own tile (mmi_lm::Td): two 16-row batch tiles at 17..32 sessions.  Needs the grouped depformer_in
    // (its row-major output is the boundary between the two tiles) and bf16 weights (the int8 / fp8 forms of the 16-row kernels
    // are instantiated for one batch tile only)
    lm->Td = lm->T;
    if (lm->T == 32 && max_batch <= 32 && lm->q8 == 0 && lm->dep_in_grouped && dd % 16 == 0 && knobs.dep_tile == 16) lm->Td = 16;
    const int Td = lm->Td;
    for (int k = 0; k < c.dep_q; ++k)
        if ((rc = load_linear(lm, W, "linears." + std::to_string(k) + ".weight", c.card, dd, 0, &lm->dep_lin[k], nullptr, nullptr, nullptr, Td))) return fail(rc);
    lm->dep_layers.resize(c.depformer_num_layers);
    for (int l = 0; l < c.depformer_num_layers; ++l) {
        DepLayerW& L = lm->dep_layers[l];
        std::string p = "depformer.layers." + std::to_string(l);
        L.in_proj.resize(c.dep_q); L.out_proj.resize(c.dep_q); L.ffn_in.resize(c.dep_q); L.ffn_out.resize(c.dep_q);
        for (int k = 0; k < nw; ++k) {
            std::string ks = std::to_string(k);
            if ((rc = load_linear(lm, W, p + ".self_attn.in_projs." + ks + ".weight", 3 * dd, dd, 0, &L.in_proj[k], nullptr, nullptr, nullptr, Td))) return fail(rc);
            if ((rc = load_linear(lm, W, p + ".self_attn.out_projs." + ks + ".weight", dd, dd, 0, &L.out_proj[k], nullptr, nullptr, nullptr, Td))) return fail(rc);
            if ((rc = load_linear(lm, W, p + ".gating." + ks + ".linear_in.weight", 2 * c.depformer_ffn_hidden, dd, c.depformer_ffn_hidden, &L.ffn_in[k], nullptr, nullptr, nullptr, Td))) return fail(rc);
            if ((rc = load_linear(lm, W, p + ".gating." + ks + ".linear_out.weight", dd, c.depformer_ffn_hidden, 0, &L.ffn_out[k], nullptr, nullptr, nullptr, Td))) return fail(rc);
        }
        {   // the sets were loaded at indices 0..nw-1; step k aliases set sched[k]
            const DepLayerW sets = L;
            for (int k = 0; k < c.dep_q; ++k) {
                L.in_proj[k] = sets.in_proj[sched[k]]; L.out_proj[k] = sets.out_proj[sched[k]];
                L.ffn_in[k] = sets.ffn_in[sched[k]]; L.ffn_out[k] = sets.ffn_out[sched[k]];
            }
        }
        if ((rc = load_copy(lm, W, p + ".norm1.alpha", 3, dd, &L.n1))) return fail(rc);
        if ((rc = load_copy(lm, W, p + ".norm2.alpha", 3, dd, &L.n2))) return fail(rc);
    }
    if ((low_rank || demux) && lm->q8 > 0)   // the reference would quantise `low_rank` / `out1` / `out2` as well (utils/quantize.py)
        return fail(mmi_fail(MMI_ERR_UNSUPPORTED, "quantised linears with low-rank or demuxed embeddings are not supported"));
    if (hipSuccess != lm->wts.alloc(&lm->delays_dev, (size_t)lm->NC)) return fail(mmi_fail(MMI_ERR_HIP, "out of device memory"));
    if (hipSuccess != hipMemcpy(lm->delays_dev, c.delays, lm->NC * sizeof(int), hipMemcpyHostToDevice)) return fail(mmi_fail(MMI_ERR_HIP, "memcpy"));
    if (hipDeviceSynchronize() != hipSuccess) return fail(mmi_fail(MMI_ERR_HIP, "weight packing failed"));
    if (lm->use_graph && hipStreamCreate(&lm->cap_stream) != hipSuccess) return fail(mmi_fail(MMI_ERR_HIP, "hipStreamCreate failed"));
    *out = lm;
    return MMI_OK;
}

extern "C" void mmi_lm_destroy(mmi_lm* lm) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return;
    mmi_lm_streaming_stop(lm);
    lm->lora_mem.release();
    lm->wts.release();
    for (auto& e : lm->ev_pool) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    for (auto& e : lm->site_ev) { if (e.ev) hipEventDestroy(e.ev); }
    if (lm->cap_stream) hipStreamDestroy(lm->cap_stream);
    delete lm;
}

extern "C" int mmi_lm_get_cfg(const mmi_lm* lm, mmi_lm_cfg* out) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !out) return mmi_fail(MMI_ERR_INVALID, "null argument");
    *out = lm->cfg;
    return MMI_OK;
}

// ---- chunked prefill -------------------------------------------------------------------------------------------
// bytes of one ring row / of its scale bytes in ring form kvf
static size_t pf_row_bytes(int kvf, int Dh) { return kvf == 2 ? Dh / 2 : (kvf == 1 ? Dh : 2 * Dh); }

// what a handle must be to prefill at all (mmi_lm_enable_prefill), and what may have changed since (mmi_lm_prefill)
static int prefill_refusal(const mmi_lm* lm, int rows) {
    const mmi_lm_cfg& c = lm->cfg;
    const int Dh = c.num_heads > 0 ? c.dim / c.num_heads : 0;
    if (rows > 128) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: a pass holds at most 128 rows");
    if (rows > 32 && lm->T == 16)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: a handle whose weights are packed at the 16-row tile (max_batch <= 16) runs passes of at most 32 rows");
    if (lm->q8 > 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: quantised linears (int8, fp8, MXFP4) are not supported: the many-row GEMM is bf16");
    if (c.cross_attention) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: models with cross-attention layers are not supported");
    if (lm->lora_on) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: adapter handles are not supported");
    if (lm->tts_on) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: a handle with the TTS machine enabled is not supported (its script state advances per step)");
    if (Dh != 32 && Dh != 64 && Dh != 128) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: head dim must be 32, 64 or 128");
    return MMI_OK;
}

// what a handle must be to score (mmi_lm_enable_score; checked again when the scratch is allocated)
static int score_refusal(const mmi_lm* lm) {
    const mmi_lm_cfg& c = lm->cfg;
    if (lm->prefill_rows <= 0) return mmi_fail(MMI_ERR_STATE, "mmi_lm_enable_score: call mmi_lm_enable_prefill first (scoring runs on the prefill pass)");
    if (c.dep_q > 0 && (lm->demux || lm->text_emb2 || lm->dep_low_rank))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "score: low-rank or demuxed depformer embeddings are not supported");
    if (c.dep_q > 0 && mmi_cdiv(lm->prefill_rows, lm->Td) > (lm->Td == 32 ? 4 : 2))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "score: the depth transformer on its own 16-row tile (MMI_DEP_TILE) runs passes of at most 32 rows");
    if (c.text_card_out % 8 || c.text_card_out > 8 * MMI_SCORE_THREADS * MMI_SCORE_PIECES || (c.dep_q > 0 && (c.card % 8 || c.card > 8 * MMI_SCORE_THREADS * MMI_SCORE_PIECES)))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "score: a head's width must be a multiple of 8 and at most 32768");
    return MMI_OK;
}

// Allocates entries [from, end) of `t` in `A`, in the table's order, hands every member its pointer and starts the fills on s
static int alloc_table(MmiArena& A, BufTable& t, size_t from, hipStream_t s, const char* what) {
    for (size_t i = from; i < t.size(); ++i) {
        BufDecl& e = t[i];
        const size_t nb = (e.count + e.tail) * e.elem;
        e.off = A.bytes;
        e.size = nb ? nb : e.elem;
        if (A.alloc(reinterpret_cast<uint8_t**>(e.slot), e.size) != hipSuccess)
            return mmi_fail(MMI_ERR_HIP, std::string("out of device memory (") + what + ")");
    }
    for (size_t i = from; i < t.size(); ++i) {
        const BufDecl& e = t[i];
        const size_t n = e.count + e.tail;
        if (e.init == BufDecl::BYTES) MMI_HIP_CHECK(hipMemsetAsync(*e.slot, e.value, n * e.elem, s));
        if (e.init == BufDecl::I32) MMI_LAUNCH(k_fill_i32, mmi_cdiv((int)n, 256), 256, 0, s, (int*)*e.slot, e.value, (long)n);
    }
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// The scoring scratch, beside the prefill scratch in its arena (outside the streaming-state arena).  Packed activations start as
// zeros: the padding rows / columns of a fragment are never written and must read as zero.
static void score_table(mmi_lm* lm, BufTable& t) {
    const mmi_lm_cfg& c = lm->cfg;
    const int rows = lm->prefill_rows, d = c.dim, dd = c.depformer_dim, q = c.dep_q;
    const size_t mt = (size_t)mmi_cdiv(rows, lm->T), mtd = (size_t)mmi_cdiv(rows, lm->Td);
    auto packed_d = [&](int features) { return mtd * packed_ksteps_t(lm, lm->Td, features) * 512; };
    auto& S = lm->sc;
    t.add(&S.tout, mt * packed_ksteps(lm, d) * 512, "sc.tout").fill(0);
    t.add(&S.tlog, (size_t)rows * c.text_card_out, "sc.tlog");
    t.add(&S.targets, (size_t)rows * (1 + q), "sc.targets");
    if (q == 0) return;
    const size_t dkv = (size_t)c.depformer_num_layers * rows * dd * q;       // [layers][rows][Hd][dep_q][Dhd]
    t.add(&S.dpre, (size_t)rows * dd, "sc.dpre");
    t.add(&S.dx, packed_d(dd), "sc.dx").fill(0);
    t.add(&S.dxn, packed_d(dd), "sc.dxn").fill(0);
    t.add(&S.datt, packed_d(dd), "sc.datt").fill(0);
    t.add(&S.dhb, packed_d(c.depformer_ffn_hidden), "sc.dhb").fill(0);
    t.add(&S.dqkv, (size_t)rows * 3 * dd, "sc.dqkv");
    t.add(&S.dkc, dkv, "sc.dkc");
    t.add(&S.dvc, dkv, "sc.dvc");
    t.add(&S.alog, (size_t)q * rows * c.card, "sc.alog");
}

static void prefill_table(mmi_lm* lm, BufTable& t) {
    const mmi_lm_cfg& c = lm->cfg;
    const int rows = lm->prefill_rows, d = c.dim, H = c.num_heads, Dh = d / H;
    const size_t mtiles = (size_t)mmi_cdiv(rows, lm->T), staged = (size_t)rows * H * pf_row_bytes(lm->ring.form, Dh);
    auto packed = [&](int features) { return mtiles * packed_ksteps(lm, features) * 512; };
    auto& P = lm->pf;
    t.add(&P.tokens, (size_t)rows * lm->NC, "pf.tokens");
    t.add(&P.row_sess, (size_t)rows, "pf.row_sess");
    t.add(&P.row_pos, (size_t)rows, "pf.row_pos");
    t.add(&P.rope, (size_t)rows * Dh, "pf.rope");
    t.add(&P.x, packed(d), "pf.x").fill(0);
    t.add(&P.xn, packed(d), "pf.xn").fill(0);
    t.add(&P.att, packed(d), "pf.att").fill(0);
    t.add(&P.hb, packed(c.ffn_hidden), "pf.hb").fill(0);
    t.add(&P.qkv, (size_t)rows * 3 * d, "pf.qkv");
    t.add(&P.q, (size_t)rows * d, "pf.q");
    t.add(&P.sk, staged, "pf.sk");
    t.add(&P.sv, staged, "pf.sv");
    t.add(&P.sks, (size_t)rows * H * (Dh / 16), "pf.sks");
    t.add(&P.svs, (size_t)rows * H * (Dh / 16), "pf.svs");
    t.add(&P.partial, (size_t)4 * rows * d, "pf.partial");
}

// the float rings of an enabled handle's stream: an arena of its own, see mmi_lm::lp_mem
static int logprobs_alloc(mmi_lm* lm, hipStream_t s) {
    const size_t n = (size_t)lm->gen_batch * (1 + lm->cfg.dep_q) * lm->CT;
    LpRings r{nullptr, nullptr, nullptr, 1 + lm->cfg.dep_q, lm->lp_top_n};
    lm->lp_mem.poison = lm->st.poison;
    hipError_t e = lm->lp_mem.alloc(&r.lp, n);
    if (e == hipSuccess && r.top_n) e = lm->lp_mem.alloc(&r.top_id, n * r.top_n);
    if (e == hipSuccess && r.top_n) e = lm->lp_mem.alloc(&r.top_lp, n * r.top_n);
    if (e != hipSuccess) return mmi_fail(MMI_ERR_HIP, "out of device memory (log-probability rings)");
    lm->lp = r;
    return clear_logprobs(lm, s, nullptr);
}

// the scratch of a stream's prefill passes (and of its scoring): an arena of its own, see mmi_lm::pf_mem
static int prefill_alloc(mmi_lm* lm, hipStream_t s) {
    int rc = prefill_refusal(lm, lm->prefill_rows);           // (adapters or the TTS machine may have been enabled after the prefill was)
    if (rc) return rc;
    lm->pf_mem.poison = lm->st.poison;
    prefill_table(lm, lm->pf_table);
    if ((rc = alloc_table(lm->pf_mem, lm->pf_table, 0, s, "prefill scratch")) || !lm->score_on) return rc;
    if ((rc = score_refusal(lm))) return rc;
    const size_t from = lm->pf_table.size();
    score_table(lm, lm->pf_table);
    return alloc_table(lm->pf_mem, lm->pf_table, from, s, "score scratch");
}

template <int KVF>
static int launch_attn_prefill_f(hipStream_t s, const PfAttnArgs& a, int Dh) {
    const dim3 grid(a.n * mmi_cdiv(a.F, MMI_PF_QT), a.H);
    switch (Dh) {
        case 128: MMI_LAUNCH((k_lm_attn_prefill<128, KVF>), grid, 256, 0, s, a); break;
        case 64: MMI_LAUNCH((k_lm_attn_prefill<64, KVF>), grid, 256, 0, s, a); break;
        case 32: MMI_LAUNCH((k_lm_attn_prefill<32, KVF>), grid, 256, 0, s, a); break;
        default: return mmi_fail(MMI_ERR_UNSUPPORTED, "head dim must be 32, 64 or 128");
    }
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}
// the attention op of a prefill pass (and mmi_lm_debug_prefill_attn)
static int launch_attn_prefill(hipStream_t s, const PfAttnArgs& a, int kvf, int Dh) {
    if (kvf == 2) return launch_attn_prefill_f<2>(s, a, Dh);
    if (kvf == 1) return launch_attn_prefill_f<1>(s, a, Dh);
    return launch_attn_prefill_f<0>(s, a, Dh);
}

// One linear of a pass on `rows` rows: launch_gemm's own selection at that row count (k_gemm_rows above 64, k_gemm_xp / k_gemm_xlds
// at or below)
static int pf_gemm(mmi_lm* lm, hipStream_t s, const GemmW& g, int rows, const uint16_t* x, int epi, const GemmOut& out, const uint16_t* resid = nullptr) {
    GemmArgs a = gemm_args(lm, g.T, x, epi, rows, rows, out, resid);
    if (epi == MMI_EPI_PARTIAL) a.partial = lm->pf.partial;
    return launch_gemm(lm, s, g, a, false);
}
// x += linear(in), in place or as split-K partials for the next norm launch to fold (add_gemm_resid's rule); returns the partials
static int pf_gemm_resid(mmi_lm* lm, hipStream_t s, const GemmW& g, int rows, const uint16_t* in, int* pending) {
    const GemmPlan p = plan_gemm(lm->knobs, g, true);
    if (p.ksplit > 4) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: the split-K partials hold at most 4 parts (MMI_GEMM_KSPLIT)");     // pf.partial is [4][rows][dim]
    *pending = p.ksplit > 1 ? p.ksplit : 0;
    if (p.ksplit <= 1) return pf_gemm(lm, s, g, rows, in, MMI_EPI_RESID, {lm->pf.x, lm->cfg.dim, true}, lm->pf.x);
    return pf_gemm(lm, s, g, rows, in, MMI_EPI_PARTIAL, {nullptr, lm->cfg.dim, true});
}
// pf.x (+= the `pending` split-K partials), y = rms_norm(pf.x) * alpha: into pf.xn, or the last norm of a scoring pass into sc.tout
static int pf_norm(mmi_lm* lm, hipStream_t s, int rows, int pending, const uint16_t* alpha, uint16_t* y = nullptr) {
    const int D = lm->cfg.dim;
    return launch_rmsnorm(s, rows, lm->pf.x, lm->pf.partial, Pending{pending}, alpha, y ? y : lm->pf.xn, D, lm->T, packed_ksteps(lm, D));
}

// One pass: F frames (f0 .. f0 + F - 1 of the call's arrays) of the n sessions of `p`, eager launches on `s`
static int launch_score_rows(hipStream_t s, const ScoreArgs& a, int rows, int sites) {
    MMI_LAUNCH(k_score_logprob, dim3(rows, sites), MMI_SCORE_THREADS, 0, s, a);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// RMSNorm of the depth transformer's rows of a scoring pass (the norm launch of the step program's norm + GEMM form)
static int sc_dep_norm(mmi_lm* lm, hipStream_t s, int rows, const uint16_t* alpha) {
    const int D = lm->cfg.depformer_dim;
    return launch_rmsnorm(s, rows, lm->sc.dx, nullptr, Pending{}, alpha, lm->sc.dxn, D, lm->Td, packed_ksteps_t(lm, lm->Td, D));
}

// The tail of a scoring pass, behind out_norm: the text head, the depth transformer as dep_q micro-steps on all R rows (micro-step
// k's input token is the given one of site k, so the rows run side by side), the logit heads, and k_score_logprob - one launch for
// the text sites, one for all audio sites.  Everything lives in lm->sc; nothing of the step's state is written.
static int score_heads(mmi_lm* lm, hipStream_t s, const PfArgs& p, const int64_t* toks, const mmi_score_out* out) {
    const mmi_lm_cfg& c = lm->cfg;
    const int R = p.n * p.F, q = c.dep_q, sites = 1 + q, rows = lm->prefill_rows;
    const int dd = c.depformer_dim, Hd = c.depformer_num_heads, Dhd = q ? dd / Hd : 0;
    auto& S = lm->sc;
    int rc;
    MMI_LAUNCH(k_sc_targets, mmi_cdiv(R * sites, 256), 256, 0, s, p, sites, (const long*)toks, S.targets);
    MMI_CHECK_LAUNCH();
    if ((rc = pf_gemm(lm, s, lm->text_linear, R, S.tout, MMI_EPI_STORE, {S.tlog, c.text_card_out}))) return rc;
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = S.tlog; a.ld = c.text_card_out; a.N = c.text_card_out;
    a.targets = S.targets; a.tgt_stride = sites; a.tgt_off = 0;
    a.logp = out->logp; a.argmax = out->argmax; a.out_stride = sites; a.out_off = 0;
    a.lf32 = out->text_logits; a.lf32_row = c.text_card_out;
    a.F = p.F; a.Tall = p.T; a.f0 = p.f0;
    if ((rc = launch_score_rows(s, a, R, 1))) return rc;
    if (q == 0) return MMI_OK;
    const size_t dkv_layer = (size_t)rows * Hd * q * Dhd;
    const int dks = packed_ksteps_t(lm, lm->Td, dd);
    for (int k = 0; k < q; ++k) {
        if ((rc = pf_gemm(lm, s, lm->dep_in[k], R, S.tout, MMI_EPI_STORE, {S.dpre, dd}))) return rc;
        ScDepInArgs in;
        in.pre = S.dpre; in.ld = dd; in.emb = lm->dep_emb[k]; in.targets = S.targets; in.sites = sites; in.site = k;
        in.out = S.dx; in.D = dd; in.T = lm->Td; in.ksteps = dks;
        MMI_LAUNCH(k_sc_dep_input, R, 128, 0, s, in);
        MMI_CHECK_LAUNCH();
        for (int l = 0; l < c.depformer_num_layers; ++l) {
            const DepLayerW& L = lm->dep_layers[l];
            if ((rc = sc_dep_norm(lm, s, R, L.n1))) return rc;
            if ((rc = pf_gemm(lm, s, L.in_proj[k], R, S.dxn, MMI_EPI_STORE, {S.dqkv, 3 * dd}))) return rc;
            DepAttnArgs da;
            da.qkv = S.dqkv; da.kc = S.dkc + l * dkv_layer; da.vc = S.dvc + l * dkv_layer; da.out = S.datt;
            da.B = R; da.H = Hd; da.Dh = Dhd; da.steps = q; da.k = k;
            da.T = lm->Td; da.out_ksteps = dks;
            if ((rc = launch_dep_attn(s, da))) return rc;
            if ((rc = pf_gemm(lm, s, L.out_proj[k], R, S.datt, MMI_EPI_RESID, {S.dx, dd, true}, S.dx))) return rc;
            if ((rc = sc_dep_norm(lm, s, R, L.n2))) return rc;
            if ((rc = pf_gemm(lm, s, L.ffn_in[k], R, S.dxn, MMI_EPI_GATE, {S.dhb, c.depformer_ffn_hidden, true}))) return rc;
            if ((rc = pf_gemm(lm, s, L.ffn_out[k], R, S.dhb, MMI_EPI_RESID, {S.dx, dd, true}, S.dx))) return rc;
        }
        if ((rc = pf_gemm(lm, s, lm->dep_lin[k], R, S.dx, MMI_EPI_STORE, {S.alog + (size_t)k * rows * c.card, c.card}))) return rc;
    }
    a.logits = S.alog; a.site_stride = (long)rows * c.card; a.ld = c.card; a.N = c.card;
    a.tgt_off = 1; a.out_off = 1;
    a.lf32 = out->audio_logits; a.lf32_row = (long)q * c.card; a.lf32_site = c.card;
    return launch_score_rows(s, a, R, q);
}

// score: null = a prefill pass.  Else the pass also runs the last layer to its end, out_norm and score_heads; commit = 0 skips
// k_pf_commit_kv and k_pf_commit_state (the attention reads the pass's own block from staging either way)
static int prefill_pass(mmi_lm* lm, hipStream_t s, PfArgs p, const int64_t* user, const int64_t* toks, const mmi_score_out* score = nullptr,
                        bool commit = true) {
    const mmi_lm_cfg& c = lm->cfg;
    const int d = c.dim, H = c.num_heads, Dh = d / H, R = p.n * p.F, n_user = c.n_q - c.dep_q, kvf = lm->ring.form;
    auto& P = lm->pf;
    TokArgs t = tok_args(lm);
    MMI_LAUNCH(k_pf_prepare, mmi_cdiv(R * lm->NC + R * (Dh / 2), 128), 128, 0, s, t, p, (const long*)user, n_user, (const long*)toks, P.tokens,
               P.row_sess, P.row_pos, P.rope, Dh, c.max_period);
    MMI_LAUNCH(k_pf_embed, dim3(mmi_cdiv(d, 256), R), 256, 0, s, (const int*)P.tokens, lm->NC, (const uint16_t*)lm->emb, c.card + 1,
               (const uint16_t*)lm->text_emb, (const uint16_t*)(lm->demux ? lm->text_emb2 : nullptr), c.text_card + 1, P.x, d, lm->T,
               packed_ksteps(lm, d), (const uint16_t*)lm->cond, (const int*)P.row_sess);
    MMI_CHECK_LAUNCH();
    const size_t kv_layer = lm->ring.layer_u16;
    int pending = 0, rc;
    for (int l = 0; l < c.num_layers; ++l) {
        const LayerW& L = lm->layers[l];
        if ((rc = pf_norm(lm, s, R, pending, L.n1))) return rc;
        if ((rc = pf_gemm(lm, s, L.in_proj, R, P.xn, MMI_EPI_STORE, {P.qkv, 3 * d}))) return rc;
        PfRopeArgs ra;
        ra.qkv = P.qkv; ra.rope = P.rope; ra.q = P.q; ra.sk = P.sk; ra.sv = P.sv; ra.sks = P.sks; ra.svs = P.svs; ra.R = R; ra.H = H; ra.Dh = Dh;
        const int rblocks = (int)mmi_cdiv64((int64_t)R * 3 * d / 16, 256);
        if (kvf == 2) MMI_LAUNCH(k_pf_rope_kv<2>, rblocks, 256, 0, s, ra);
        else if (kvf == 1) MMI_LAUNCH(k_pf_rope_kv<1>, rblocks, 256, 0, s, ra);
        else MMI_LAUNCH(k_pf_rope_kv<0>, rblocks, 256, 0, s, ra);
        MMI_CHECK_LAUNCH();
        PfAttnArgs a;
        memset(&a, 0, sizeof(a));
        a.q = P.q; a.kc = reinterpret_cast<uint8_t*>(lm->kc + l * kv_layer); a.vc = reinterpret_cast<uint8_t*>(lm->vc + l * kv_layer);
        a.kv_soff = (long)lm->ring.scale_off;
        a.sk = P.sk; a.sv = P.sv; a.sks = P.sks; a.svs = P.svs; a.row_sess = P.row_sess; a.row_pos = P.row_pos;
        a.out = P.att; a.T = lm->T; a.out_ksteps = packed_ksteps(lm, d);
        a.H = H; a.cap = c.context; a.context = c.context; a.n = p.n; a.F = p.F;
        const bool last = l + 1 == c.num_layers;        // the last layer's attention output, FFN and out_norm feed nothing
        if ((!last || score) && (rc = launch_attn_prefill(s, a, kvf, Dh))) return rc;
        const int cblocks = (int)mmi_cdiv64((int64_t)R * H * (pf_row_bytes(kvf, Dh) / 16), 256);
        if (commit) {
            if (kvf == 2) MMI_LAUNCH(k_pf_commit_kv<2>, cblocks, 256, 0, s, a, Dh);
            else if (kvf == 1) MMI_LAUNCH(k_pf_commit_kv<1>, cblocks, 256, 0, s, a, Dh);
            else MMI_LAUNCH(k_pf_commit_kv<0>, cblocks, 256, 0, s, a, Dh);
            MMI_CHECK_LAUNCH();
        }
        if (last && !score) break;
        if ((rc = pf_gemm_resid(lm, s, L.out_proj, R, P.att, &pending))) return rc;
        if ((rc = pf_norm(lm, s, R, pending, L.n2))) return rc;
        if ((rc = pf_gemm(lm, s, L.ffn_in, R, P.xn, MMI_EPI_GATE, {P.hb, c.ffn_hidden, true}))) return rc;
        if ((rc = pf_gemm_resid(lm, s, L.ffn_out, R, P.hb, &pending))) return rc;
    }
    if (score) {
        if ((rc = pf_norm(lm, s, R, pending, lm->out_norm, lm->sc.tout))) return rc;
        if ((rc = score_heads(lm, s, p, toks, score))) return rc;
    }
    if (!commit) return MMI_OK;
    MMI_LAUNCH(k_pf_commit_state, mmi_cdiv(p.n, 64), 64, 0, s, t, p, (const long*)user, n_user, (const long*)toks, lm->text_tok, lm->audio_tok);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

extern "C" int mmi_lm_enable_prefill(mmi_lm* lm, int32_t rows) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "mmi_lm_enable_prefill: not while streaming");
    if (rows < 0) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_enable_prefill: rows must be 0 (off) or 1..128");
    if (rows > 0) {
        const int rc = prefill_refusal(lm, rows);
        if (rc) return rc;
    }
    lm->prefill_rows = rows;
    return MMI_OK;
}

extern "C" int32_t mmi_lm_prefill_rows(const mmi_lm* lm) {
    if (!lm) return (int32_t)mmi_fail(MMI_ERR_INVALID, "null handle");
    return lm->prefill_rows;
}

extern "C" int mmi_lm_prefill(mmi_lm* lm, const int32_t* sessions, int32_t n, const int64_t* user_codes, const int64_t* tokens, int32_t T,
                              mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !sessions || !tokens) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if (lm->prefill_rows <= 0 || !lm->pf.x)
        return mmi_fail(MMI_ERR_STATE, "prefill is not enabled: call mmi_lm_enable_prefill before streaming_start");
    const mmi_lm_cfg& c = lm->cfg;
    if (!user_codes && c.n_q > c.dep_q) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (T < 1) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_prefill: T must be >= 1");
    if (n < 1 || n > lm->prefill_rows) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_prefill: 1 .. prefill_rows sessions per call");
    PfArgs p;
    memset(&p, 0, sizeof(p));
    std::vector<uint8_t> seen(lm->gen_batch, 0);
    for (int i = 0; i < n; ++i) {
        if (sessions[i] < 0 || sessions[i] >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_prefill: session index out of range");
        if (seen[sessions[i]]) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_prefill: a session is named twice");
        seen[sessions[i]] = 1;
        p.sess[i] = (uint8_t)sessions[i];
    }
    // what a stream or a step may have brought since the prefill was enabled
    if (lm->cfg_coef != 1.f || lm->batch != lm->gen_batch) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: a guided stream (guidance twins) is not supported");
    if (lm->hooks.on_text_logits || lm->hooks.on_text_token || lm->hooks.on_audio_tokens)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: not while per-step hooks are installed");
    if (lm->tts || lm->lora_on) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: not on a stream with the TTS machine or adapters");
    hipStream_t s = (hipStream_t)stream;
    p.n = n; p.T = T;
    const int F = lm->prefill_rows / n;
    for (int f0 = 0; f0 < T; f0 += F) {
        p.f0 = f0;
        p.F = T - f0 < F ? T - f0 : F;
        const int rc = prefill_pass(lm, s, p, user_codes, tokens);
        if (rc) return rc;
    }
    if (const int rc = clear_logprobs(lm, s, nullptr, p.sess, n)) return rc;      // given tokens: nothing was sampled
    lm->offset_cpu += T;
    if (lm->depth_bound < (1L << 40)) lm->depth_bound += T;
    return MMI_OK;
}

// ---- teacher-forced scoring on the prefill path ---------------------------------------------------------------
extern "C" int mmi_lm_enable_score(mmi_lm* lm, int32_t on) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "mmi_lm_enable_score: not while streaming");
    if (on) {
        const int rc = score_refusal(lm);
        if (rc) return rc;
    }
    lm->score_on = on != 0;
    return MMI_OK;
}

extern "C" int32_t mmi_lm_score_enabled(const mmi_lm* lm) {
    if (!lm) return (int32_t)mmi_fail(MMI_ERR_INVALID, "null handle");
    return lm->score_on ? 1 : 0;
}

extern "C" int mmi_lm_score(mmi_lm* lm, const int32_t* sessions, int32_t n, const int64_t* user_codes, const int64_t* tokens, int32_t T,
                            int32_t commit, const mmi_score_out* out, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !sessions || !tokens || !out) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if (!lm->score_on || lm->prefill_rows <= 0 || !lm->sc.tout)
        return mmi_fail(MMI_ERR_STATE, "score is not enabled: call mmi_lm_enable_prefill and mmi_lm_enable_score before streaming_start");
    const mmi_lm_cfg& c = lm->cfg;
    if (!user_codes && c.n_q > c.dep_q) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!out->logp) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_score: out->logp must not be null");
    if (T < 1) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_score: T must be >= 1");
    if (n < 1 || n > lm->prefill_rows) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_score: 1 .. prefill_rows sessions per call");
    PfArgs p;
    memset(&p, 0, sizeof(p));
    std::vector<uint8_t> seen(lm->gen_batch, 0);
    for (int i = 0; i < n; ++i) {
        if (sessions[i] < 0 || sessions[i] >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_score: session index out of range");
        if (seen[sessions[i]]) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_score: a session is named twice");
        seen[sessions[i]] = 1;
        p.sess[i] = (uint8_t)sessions[i];
    }
    if (!commit && (long)n * T > lm->prefill_rows)
        return mmi_fail(MMI_ERR_INVALID, "mmi_lm_score: commit = 0 must fit one pass (n * T <= prefill_rows): a later pass would need the earlier one's K/V in the ring");
    // prefill's own refusals, in its words
    if (lm->cfg_coef != 1.f || lm->batch != lm->gen_batch) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: a guided stream (guidance twins) is not supported");
    if (lm->hooks.on_text_logits || lm->hooks.on_text_token || lm->hooks.on_audio_tokens)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: not while per-step hooks are installed");
    if (lm->tts || lm->lora_on) return mmi_fail(MMI_ERR_UNSUPPORTED, "prefill: not on a stream with the TTS machine or adapters");
    hipStream_t s = (hipStream_t)stream;
    p.n = n; p.T = T;
    const int F = lm->prefill_rows / n;
    for (int f0 = 0; f0 < T; f0 += F) {
        p.f0 = f0;
        p.F = T - f0 < F ? T - f0 : F;
        const int rc = prefill_pass(lm, s, p, user_codes, tokens, out, commit != 0);
        if (rc) return rc;
    }
    if (commit) {
        if (const int rc = clear_logprobs(lm, s, nullptr, p.sess, n)) return rc;
        lm->offset_cpu += T;
        if (lm->depth_bound < (1L << 40)) lm->depth_bound += T;
    }
    return MMI_OK;
}

// Parity tap of the scoring output kernel (include/moshi_mi.h): k_score_logprob alone through the pass's launch function
extern "C" int mmi_lm_debug_score_rows(mmi_lm* lm, const void* logits_bf16, const int32_t* targets, int32_t rows, int32_t N, float* logp,
                                       int32_t* argmax, float* logits_f32, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !logits_bf16 || !targets || !logp || !argmax) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (rows < 1 || rows > (1 << 20)) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_score_rows: 1 <= rows <= 2^20");
    if (N < 8 || N % 8 || N > 8 * MMI_SCORE_THREADS * MMI_SCORE_PIECES)
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_score_rows: N must be a multiple of 8 in [8, 32768]");
    if ((uintptr_t)logits_bf16 % 16 || (uintptr_t)logits_f32 % 16 || (uintptr_t)targets % 4 || (uintptr_t)logp % 4 || (uintptr_t)argmax % 4)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_score_rows: the logits must be 16-byte aligned");
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = (const uint16_t*)logits_bf16; a.ld = N; a.N = N;
    a.targets = targets; a.tgt_stride = 1;
    a.logp = logp; a.argmax = argmax; a.out_stride = 1;
    a.lf32 = logits_f32; a.lf32_row = N;
    a.F = rows; a.Tall = rows; a.f0 = 0;
    return launch_score_rows((hipStream_t)stream, a, rows, 1);
}

extern "C" int mmi_lm_last_tokens(mmi_lm* lm, int64_t* out, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !out) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    const int G = lm->gen_batch, q = lm->cfg.dep_q;
    MMI_LAUNCH(k_pf_last_tokens, mmi_cdiv(G * (1 + q), 256), 256, 0, (hipStream_t)stream, (const int*)lm->text_tok, (const int*)lm->audio_tok, G, q, (long*)out);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// ---- log-probabilities in the live step -------------------------------------------------------------------------
extern "C" int mmi_lm_enable_logprobs(mmi_lm* lm, int32_t on, int32_t top_n) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (top_n < 0 || top_n > MMI_LP_MAX_TOP) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_enable_logprobs: top_n must lie in [0, 8]");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "mmi_lm_enable_logprobs: not while streaming");
    lm->lp_on = on != 0;
    lm->lp_top_n = on ? top_n : 0;
    return MMI_OK;
}

extern "C" int mmi_lm_logprobs_enabled(const mmi_lm* lm, int32_t* top_n_or_null) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (top_n_or_null) *top_n_or_null = lm->lp_top_n;
    return lm->lp_on ? 1 : 0;
}

static int read_logprobs(mmi_lm* lm, const char* who, int frame, float* logp, int32_t* top_id, float* top_logp, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!logp) return mmi_fail(MMI_ERR_INVALID, std::string(who) + ": logp must not be null");
    if (!lm->lp_on) return mmi_fail(MMI_ERR_STATE, std::string(who) + ": log-probabilities are not enabled (mmi_lm_enable_logprobs before streaming_start)");
    if (!lm->streaming || !lm->lp.lp) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if ((top_id || top_logp) && lm->lp.top_n == 0)
        return mmi_fail(MMI_ERR_INVALID, std::string(who) + ": the handle records no alternatives (top_n == 0)");
    if ((top_id == nullptr) != (top_logp == nullptr)) return mmi_fail(MMI_ERR_INVALID, std::string(who) + ": top_id and top_logp go together");
    const int n = lm->gen_batch * lm->lp.sites;
    MMI_LAUNCH(k_lp_read, mmi_cdiv(n, 256), 256, 0, (hipStream_t)stream, tok_args(lm), lm->lp, (const int*)lm->out_i32, frame, logp, top_id, top_logp);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

extern "C" int mmi_lm_last_logprobs(mmi_lm* lm, float* logp, int32_t* top_id, float* top_logp, mmi_stream stream) {
    return read_logprobs(lm, "mmi_lm_last_logprobs", 0, logp, top_id, top_logp, stream);
}

extern "C" int mmi_lm_frame_logprobs(mmi_lm* lm, float* logp, int32_t* top_id, float* top_logp, mmi_stream stream) {
    return read_logprobs(lm, "mmi_lm_frame_logprobs", 1, logp, top_id, top_logp, stream);
}

// The regions of the streaming-state arena (mmi_lm_state_save's buffer) by name: "name<TAB>offset<TAB>bytes<TAB>rows<TAB>kind" per
// line.  rows > 0: the region is `rows` equal slices, one per session (model row); kind 1 = state that the next step reads (what a
// session IS), 0 = scratch that every step rewrites before reading it.
extern "C" int64_t mmi_lm_debug_state_regions(const mmi_lm* lm, char* buf, int64_t cap) {
    if (!lm || !lm->streaming) return 0;
    const BufTable& t = lm->st_table;
    const KvRing& ring = lm->ring;
    std::string text;
    auto line = [&](const std::string& name, size_t off, size_t bytes, int rows, int kind) {
        text += name + "\t" + std::to_string(off) + "\t" + std::to_string(bytes) + "\t" + std::to_string(rows) + "\t" + std::to_string(kind) + "\n";
    };
    int last = 0;
    for (const BufDecl& e : t) last = e.late > last ? e.late : last;
    for (int pass = 0; pass <= last; ++pass)
        for (const BufDecl& e : t) {
            if (e.kind != 1 || e.late != pass) continue;
            if (e.slot != (void**)&lm->kc && e.slot != (void**)&lm->vc) { line(e.name, e.off, e.count * e.elem, e.rows, 1); continue; }
            for (int l = 0; l < lm->cfg.num_layers; ++l) {   // a ring, layer by layer (a 4-bit layer: codes plane, then scale plane)
                const std::string nm = std::string(e.name) + "." + std::to_string(l);
                const size_t off = e.off + l * ring.layer_u16 * sizeof(uint16_t);
                line(nm, off, ring.codes_bytes, e.rows, 1);
                if (ring.form == 2) line(nm + ".scale", off + ring.scale_off, ring.elems / 16, e.rows, 1);
            }
        }
    for (size_t i = 0; i < t.size(); ++i)
        if (t[i].kind == 0) line("scratch" + std::to_string(i), t[i].off, t[i].size, 0, 0);
    const int64_t need = (int64_t)text.size() + 1;
    if (buf && cap >= need) memcpy(buf, text.c_str(), (size_t)need);
    return need;
}

// The scratch of a parity tap (mmi_lm_debug_*): an arena of its own - a streaming session is not disturbed - under the handle's
// poison knob.  Leaving the tap by ANY return drains the stream and releases the arena, so the taps use the ordinary
// MMI_HIP_CHECK / MMI_CHECK_LAUNCH early returns.
namespace {
struct TapScratch {
    MmiArena A;
    hipStream_t s;
    const char* tap;      // the entry's name, for the texts of HIP failures
    TapScratch(const mmi_lm* lm, hipStream_t stream, const char* name) : s(stream), tap(name) { A.poison = lm->knobs.debug_poison; }
    TapScratch(const TapScratch&) = delete;
    TapScratch& operator=(const TapScratch&) = delete;
    ~TapScratch() {
        hipStreamSynchronize(s);
        A.release();
    }
    template <class T>
    int alloc(T** p, size_t n) {
        if (A.alloc(p, n) != hipSuccess) return mmi_fail(MMI_ERR_HIP, std::string("out of device memory (") + tap + ")");
        return MMI_OK;
    }
    template <class T>
    int zeroed(T** p, size_t n) {
        const int rc = alloc(p, n);
        if (rc) return rc;
        MMI_HIP_CHECK(hipMemsetAsync(*p, 0, n * sizeof(T), s));
        return MMI_OK;
    }
    // a zeroed packed tensor of rows x d at tile T (the padding rows and columns of a packed operand read as zero)
    int packed(uint16_t** p, int rows, int T, int ksteps) { return zeroed(p, (size_t)mmi_cdiv(rows, T) * ksteps * 512); }
    // ... unpacked into the caller's row-major [rows][d], and the tap's launches waited for
    int unpack(const uint16_t* p, int rows, int d, int T, int ksteps, void* out_bf16) {
        MMI_LAUNCH(k_unpack_rows, mmi_cdiv(rows * d, 256), 256, 0, s, p, rows, d, (uint16_t*)out_bf16, T, ksteps);
        MMI_CHECK_LAUNCH();
        if (hipStreamSynchronize(s) != hipSuccess) return mmi_fail(MMI_ERR_HIP, std::string(tap) + ": the launches failed");
        return MMI_OK;
    }
};
}  // namespace

// Parity tap of the step's log-probability op (include/moshi_mi.h): k_step_logprob through launch_step_logprob - the launch function
// of the step program's op - on caller rows: one site of width N, every row executing, a ring of one slot, which is the caller's
// [rows] / [rows][top_n] layout.  Alternatives the caller does not take land in scratch of the tap's own.
extern "C" int mmi_lm_debug_step_logprob(mmi_lm* lm, const void* logits_bf16, const int32_t* targets, int32_t rows, int32_t N, int32_t top_n,
                                         float* logp, int32_t* top_id, float* top_logp, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !logits_bf16 || !targets) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!logp) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_step_logprob: logp must not be null");
    if (top_n < 0 || top_n > MMI_LP_MAX_TOP) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_step_logprob: top_n must lie in [0, 8]");
    if ((top_id || top_logp) && top_n == 0) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_step_logprob: no alternatives were asked for (top_n == 0)");
    if (rows < 1 || rows > (1 << 20)) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_step_logprob: 1 <= rows <= 2^20");
    if (N < 8 || N % 8 || N > 8 * MMI_SCORE_THREADS * MMI_SCORE_PIECES)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_step_logprob: N must be a multiple of 8 in [8, 32768]");
    if ((uintptr_t)logits_bf16 % 16 || (uintptr_t)targets % 4 || (uintptr_t)logp % 4 || (uintptr_t)top_id % 4 || (uintptr_t)top_logp % 4)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_step_logprob: the logits must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    TapScratch scratch(lm, s, "mmi_lm_debug_step_logprob");
    int rc;
    if (top_n && !top_id && (rc = scratch.alloc(&top_id, (size_t)rows * top_n))) return rc;
    if (top_n && !top_logp && (rc = scratch.alloc(&top_logp, (size_t)rows * top_n))) return rc;
    LpArgs a;
    memset(&a, 0, sizeof(a));
    a.t.CT = 1; a.t.B = rows;
    a.text_logits = (const uint16_t*)logits_bf16; a.text_N = N;
    a.text_tok = targets;
    a.r = LpRings{logp, top_id, top_logp, 1, top_n};
    return launch_step_logprob(s, a, rows);
}

// Parity tap of the prefill attention (include/moshi_mi.h): launch_attn_prefill - the attention op of a pass - on caller-supplied
// operands, with a packed output of its own.  Nothing of the handle but its device and its poison knob is read.
extern "C" int mmi_lm_debug_prefill_attn(mmi_lm* lm, const void* q_bf16, const int32_t* row_ring, const int64_t* row_pos, const void* k_ring,
                                         const void* v_ring, const void* k_staged, const void* v_staged, int32_t rows, int32_t n_blocks,
                                         int32_t rings, int32_t H, int32_t Dh, int32_t cap, int32_t context, int32_t kv_dtype, void* out_bf16,
                                         mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !q_bf16 || !row_ring || !row_pos || !k_ring || !v_ring || !k_staged || !v_staged || !out_bf16)
        return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (kv_dtype != MMI_BF16 && kv_dtype != MMI_F8E4M3 && kv_dtype != MMI_F4E2M1X2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_prefill_attn: the ring is bf16, e4m3 or 4-bit (MMI_F4E2M1X2)");
    const int kvf = kv_form(kv_dtype);
    if (Dh != 32 && Dh != 64 && Dh != 128) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_prefill_attn: head dim must be 32, 64 or 128");
    if (rows <= 0 || rows > 128 || n_blocks <= 0 || rows % n_blocks)
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_prefill_attn: 1..128 rows in n_blocks equal blocks");
    if (H <= 0 || H > 1024 || rings <= 0 || cap <= 0 || cap > (1 << 20) || context <= 0 || context > cap)
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_prefill_attn: 1 <= H <= 1024, rings >= 1, 1 <= context <= cap <= 2^20");
    if (((uintptr_t)q_bf16 | (uintptr_t)k_ring | (uintptr_t)v_ring | (uintptr_t)k_staged | (uintptr_t)v_staged) % 16 || (uintptr_t)row_pos % 8 ||
        (uintptr_t)row_ring % 4 || (uintptr_t)out_bf16 % 2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_prefill_attn: q, the rings and the staged blocks must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int F = rows / n_blocks;
    {   // the row table must be what a pass builds: one ring per block, consecutive positions from a start >= 0
        std::vector<int32_t> rr(rows);
        std::vector<int64_t> rp(rows);
        MMI_HIP_CHECK(hipStreamSynchronize(s));
        MMI_HIP_CHECK(hipMemcpy(rr.data(), row_ring, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
        MMI_HIP_CHECK(hipMemcpy(rp.data(), row_pos, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; ++r) {
            const int r0 = r / F * F;
            if (rr[r] < 0 || rr[r] >= rings || rr[r] != rr[r0] || rp[r0] < 0 || rp[r] != rp[r0] + (r - r0))
                return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_prefill_attn: a block's rows name one ring in [0, rings) and consecutive positions >= 0");
        }
    }
    const int d = H * Dh, T = rows <= 16 ? 16 : 32, ksteps = mmi_cdiv(d, mmi_kstep(T));
    TapScratch scratch(lm, s, "mmi_lm_debug_prefill_attn");
    uint16_t* att = nullptr;
    int rc = scratch.packed(&att, rows, T, ksteps);
    if (rc) return rc;
    PfAttnArgs a;
    memset(&a, 0, sizeof(a));
    const size_t rowb = pf_row_bytes(kvf, Dh);
    a.q = (const uint16_t*)q_bf16; a.kc = (uint8_t*)k_ring; a.vc = (uint8_t*)v_ring;
    a.kv_soff = kvf == 2 ? (long)rings * H * cap * Dh / 2 : 0;
    a.sk = (const uint8_t*)k_staged; a.sv = (const uint8_t*)v_staged;
    a.sks = a.sk + (size_t)rows * H * rowb; a.svs = a.sv + (size_t)rows * H * rowb;
    a.row_sess = row_ring; a.row_pos = reinterpret_cast<const long*>(row_pos);
    a.out = att; a.T = T; a.out_ksteps = ksteps; a.H = H; a.cap = cap; a.context = context; a.n = n_blocks; a.F = F;
    if ((rc = launch_attn_prefill(s, a, kvf, Dh))) return rc;
    return scratch.unpack(att, rows, d, T, ksteps, out_bf16);
}

// The streaming-state arena of the stream being started, buffer by buffer: add(member, count, name, rows, kind), then how it starts.
// ORDER IS FORMAT: a snapshot (mmi_lm_state_save) is these buffers back to back, so a new buffer goes where its feature's
// condition puts it and nothing moves (tests/golden/lm_state_layout.json pins order, sizes and fills).
// Needs batch / gen_batch, kmax, cross_cap, act8, tts_stride and ring of the stream.  "state*": holds per-session state but is
// declared kind 0, because mmi_lm_debug_state_regions has always reported it as scratch.
static void state_table(mmi_lm* lm, const mmi_guidance* guide, bool guided, BufTable& t) {
    const mmi_lm_cfg& c = lm->cfg;
    const int G = lm->gen_batch, B = lm->batch, d = c.dim, H = c.num_heads, Dh = d / H, dd = c.depformer_dim, q = c.dep_q, T = lm->T, Td = lm->Td;
    const int NS = attn_splits(lm->knobs, c, B);
    const size_t kvn = (size_t)c.num_layers * lm->ring.layer_u16;                  // uint16 units
    const int Hd = c.depformer_num_heads, Dhd = dd / Hd;
    const size_t dkvn = (size_t)c.depformer_num_layers * B * Hd * q * Dhd;         // [dep_layers][B][Hd][dep_q][Dhd]
    t.add(&lm->exec, G, "exec", G, 1).fill(1);
    t.add(&lm->offsets, G, "offsets", G, 1).fill(0);
    if (guided) t.add(&lm->offsets_m, B, "offsets_m", B).fill(0);                                          // state*
    if (guided && guide->cfg_is_masked_until) t.add(&lm->masked_until, G, "masked_until", G);              // state*
    if (guide && guide->condition_sum) t.add(&lm->cond, (size_t)B * d, "cond", B, 1).late = 2;
    t.add(&lm->coefs, G, "coefs", G, 1).late = 1;
    if (c.cross_attention) {
        // slots [cross_len, cap) of a row are never read before mmi_lm_set_row_condition fills them: zero for the snapshot's sake
        BufDecl& xkv = t.add(&lm->xkv, (size_t)c.num_layers * B * lm->cross_cap * 2 * d, "xkv");          // state*
        if (lm->cross_cap != lm->cross_len) xkv.fill(0);
        t.add(&lm->xlen, B, "xlen", B).fill_i32(lm->cross_len);                                            // state*
    }
    t.add(&lm->cache, (size_t)G * lm->NC * lm->CT, "cache", G, 1).fill_i32(-2);                            // lm.py:608-613
    t.add(&lm->user_i32, (size_t)G * (c.n_q - q), "user_i32");
    t.add(&lm->tokens, (size_t)B * lm->NC, "tokens");
    t.add(&lm->text_tok, G, "text_tok", G, 1).fill(0);
    t.add(&lm->audio_tok, (size_t)G * q, "audio_tok", q ? G : 0, 1).fill(0);
    t.add(&lm->out_i32, (size_t)G * (q + 1), "out_i32");
    // packed activations start as zeros: the padding rows / columns of a fragment are never written and must read as zero
    t.add(&lm->x, packed_elems(lm, d), "x").fill(0);
    t.add(&lm->xn, packed_elems(lm, d), "xn").fill(0);
    t.add(&lm->qrot, (size_t)B * d, "qrot");
    t.add(&lm->att, packed_elems(lm, d), "att").fill(0);
    t.add(&lm->hb, packed_elems(lm, c.ffn_hidden), "hb").fill(0);
    t.add(&lm->tout, packed_elems(lm, d), "tout").fill(0);
    t.add(&lm->text_logits, (size_t)B * c.text_card_out, "text_logits");
    // every plane of the ring, a 4-bit ring's scale planes included: the attention reads rows past the valid length with p = 0, so
    // they must decode to finite values - scale byte 0 is the factor 0.0f, 255 would be Inf (Inf * 0 = NaN)
    t.add(&lm->kc, kvn, "kc", B, 1).fill(0).late = 3;
    t.add(&lm->vc, kvn, "vc", B, 1).fill(0).late = 3;
    t.add(&lm->opart, (size_t)B * H * NS * Dh, "opart");
    t.add(&lm->ml, (size_t)B * H * NS * 2, "ml");
    t.add(&lm->attn_done, (size_t)B * H, "attn_done").fill(0);
    t.add(&lm->partial, (size_t)4 * B * (d > dd ? d : dd), "partial");
    t.add(&lm->rope, (size_t)B * Dh, "rope");
    if (lm->hidden_taps) t.add(&lm->htap, (size_t)2 * B * d, "htap");
    if (lm->act8) {   // the int8 operands (see mmi_lm::act8): like their bf16 twins, padding rows / k-steps must read as zero
        const size_t mtiles = (size_t)mmi_cdiv(B, T), rows = mtiles * T;
        auto qbytes = [&](int features) { return mtiles * (size_t)(packed_ksteps(lm, features) / 2) * 1024; };
        t.add(&lm->xnq, qbytes(d), "xnq").fill(0);
        t.add(&lm->attq, qbytes(d), "attq").fill(0);
        t.add(&lm->hbq, qbytes(c.ffn_hidden > c.depformer_ffn_hidden ? c.ffn_hidden : c.depformer_ffn_hidden), "hbq").fill(0);
        t.add(&lm->toutq, qbytes(d), "toutq").fill(0);
        t.add(&lm->dxnq, qbytes(dd > 0 ? dd : 8), "dxnq").fill(0);
        t.add(&lm->sx_xn, rows, "sx_xn").fill(0);
        t.add(&lm->sx_tout, rows, "sx_tout").fill(0);
        t.add(&lm->sx_dxn, rows, "sx_dxn").fill(0);
        t.add(&lm->sx_att, rows, "sx_att").fill(0);
        t.add(&lm->sx_hb, rows, "sx_hb").fill(0);
    }
    t.add(&lm->dx, packed_elems_t(lm, Td, dd), "dx").fill(0);
    t.add(&lm->dxn, packed_elems_t(lm, Td, dd), "dxn").fill(0);
    t.add(&lm->dqkv, (size_t)B * 3 * dd, "dqkv");
    t.add(&lm->datt, packed_elems_t(lm, Td, dd), "datt").fill(0);
    t.add(&lm->dhb, packed_elems_t(lm, Td, c.depformer_ffn_hidden), "dhb").fill(0);
    t.add(&lm->dlogits, (size_t)q * B * c.card, "dlogits");
    t.add(&lm->dpre, (size_t)B * q * dd, "dpre");
    t.add(&lm->dkc, dkvn, "dkc").fill(0);
    t.add(&lm->dvc, dkvn, "dvc").fill(0);
    t.add(&lm->noise, (size_t)G * (1 + q) * lm->kmax, "noise");
    t.add(&lm->use_noise, 1, "use_noise").fill(0);
    t.add(&lm->forced, (size_t)G * (1 + q), "forced");
    t.add(&lm->use_forced, 1, "use_forced").fill(0);
    t.add(&lm->rng, 2, "rng", 0, 1);
    // every row inactive.  The nucleus table rides behind the row table (k_sample_nucleus finds it at rows + G): whole RowSamp
    // entries, so that the snapshot of a stream without the nucleus kernels keeps its size
    t.add(&lm->rowtab, G, "rowtab", G, 1).fill(0).tail = lm->nucleus_on ? ((size_t)G * sizeof(RowTopP) + sizeof(RowSamp) - 1) / sizeof(RowSamp) : 0;
    t.add(&lm->thist, (size_t)G * MMI_TEXT_HIST, "thist", G, 1).fill(0);
    if (lm->tts_on) t.add(&lm->tts, (size_t)G * lm->tts_stride, "tts", G).fill(0);    // state*; no session has a script: every header word 0
    if (lm->lora_on) {      // every row without an adapter; the padding rows of t are never written and must read as zero
        t.add(&lm->row_slot, G, "row_slot", G).fill_i32(-1);                           // state*
        t.add(&lm->lora_t, (size_t)mmi_cdiv(B, T) * (lm->lora_S * lm->lora_R / mmi_kstep(T)) * 512, "lora_t").fill(0);
    }
}

extern "C" int mmi_lm_streaming_start(mmi_lm* lm, int32_t batch, const mmi_sampling* sampling, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    return mmi_lm_streaming_start_guided(lm, batch, sampling, nullptr, stream);
}

extern "C" int mmi_lm_streaming_start_guided(mmi_lm* lm, int32_t batch, const mmi_sampling* sampling, const mmi_guidance* guide,
                                             mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !sampling) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "already streaming");
    const bool guided = guide && guide->cfg_coef != 1.0f;
    const int rows = guided ? 2 * batch : batch;              // lm.py:646-647 `batch_size *= 2`
    if (batch <= 0 || rows > lm->max_batch)
        return mmi_fail(MMI_ERR_SHAPE, guided ? "guidance runs two model rows per session: 2 * batch exceeds max_batch" : "batch exceeds max_batch");
    if (sampling->top_k > 256 || sampling->top_k_text > 256) return mmi_fail(MMI_ERR_UNSUPPORTED, "top_k > 256");
    if (sampling->top_k < 0 || sampling->top_k_text < 0) return mmi_fail(MMI_ERR_INVALID, "top_k must be >= 0 (0 = no top-k)");
    hipStream_t s = (hipStream_t)stream;
    const mmi_lm_cfg& c = lm->cfg;
    lm->batch = rows;
    lm->gen_batch = batch;
    lm->cfg_coef = guided ? guide->cfg_coef : 1.f;
    lm->cfg_no_text = guided && guide->cfg_is_no_text ? 1 : 0;
    lm->samp = *sampling;
    lm->kmax = sampling->top_k > sampling->top_k_text ? sampling->top_k : sampling->top_k_text;
    if (lm->kmax < 1) lm->kmax = 1;
    lm->offset_cpu = 0;
    lm->depth_bound = 0;
    lm->precapture_failed = false;
    const int G = batch, B = rows, d = c.dim;
    auto fail = [&](int code) { lm->streaming = true; mmi_lm_streaming_stop(lm); return code; };
    lm->cross_len = lm->cross_cap = 0;
    if (c.cross_attention) {
        if (!guide || !guide->condition_cross || guide->cross_len <= 0)
            return fail(mmi_fail(MMI_ERR_INVALID, "the model has cross-attention layers: mmi_guidance.condition_cross is required"));   // transformer.py:793-795
        if (lm->cross_cap_set && lm->cross_cap_set < guide->cross_len)
            return fail(mmi_fail(MMI_ERR_SHAPE, "mmi_guidance.cross_len exceeds the capacity set with mmi_lm_set_cross_capacity"));
        lm->cross_len = guide->cross_len;
        lm->cross_cap = lm->cross_cap_set ? lm->cross_cap_set : lm->cross_len;
    } else if (guide && guide->condition_cross) {
        return fail(mmi_fail(MMI_ERR_INVALID, "a cross-attention condition was given to a model without cross-attention layers"));
    }
    lm->act8 = act8_of(lm);
    lm->tts_stride = lm->tts_on ? MMI_TTS_HDR + 2 * lm->tts_max_tokens + 3 * lm->tts_max_entries + 1 + (1 + c.dep_q) * lm->tts_max_prefix : 0;
    lm->ring = kv_ring_of(c, B);
    state_table(lm, guide, guided, lm->st_table);
    int rc = alloc_table(lm->st, lm->st_table, 0, s, "LM streaming state");
    if (rc) return fail(rc);
    if (!guided) lm->offsets_m = lm->offsets;
    lm->nucleus_live = lm->nucleus_on;
    lm->row_top_p.assign(lm->nucleus_live ? G : 0, RowTopP{lm->top_p, lm->top_p_text});   // every session starts with the handle's values
    // the host's mirrors of what the fills wrote
    lm->noise_on = lm->forced_armed = false;
    lm->row_active.assign(G, 0);
    if (lm->row_slot) lm->row_slot_h.assign(G, -1);
    auto rest = [&]() -> int {      // what is left of the start; a failure leaves through fail() like every other
        // the starts that need a host image or a copy
        if (lm->masked_until) {   // host int64[batch] (LMGen(cfg_is_masked_until=[...]), lm.py:637-640)
            std::vector<int> mu(G);
            for (int i = 0; i < G; ++i) mu[i] = (int)guide->cfg_is_masked_until[i];
            MMI_HIP_CHECK(hipMemcpy(lm->masked_until, mu.data(), G * sizeof(int), hipMemcpyHostToDevice));
        }
        std::vector<float> cf(G, lm->cfg_coef);    // every session starts with the stream's coefficient
        MMI_HIP_CHECK(hipMemcpy(lm->coefs, cf.data(), G * sizeof(float), hipMemcpyHostToDevice));
        unsigned long long r0[2] = {sampling->seed, 0ull};
        MMI_HIP_CHECK(hipMemcpyAsync(lm->rng, r0, sizeof(r0), hipMemcpyHostToDevice, s));
        if (lm->nucleus_live)
            MMI_HIP_CHECK(hipMemcpyAsync(lm->rowtab + G, lm->row_top_p.data(), (size_t)G * sizeof(RowTopP), hipMemcpyHostToDevice, s));
        if (lm->cond) MMI_HIP_CHECK(hipMemcpyAsync(lm->cond, guide->condition_sum, (size_t)B * d * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
        if (lm->tts) {
            if (hipHostMalloc((void**)&lm->tts_stage, (size_t)G * lm->tts_stride * sizeof(int), 0) != hipSuccess) {
                lm->tts_stage = nullptr;
                return mmi_fail(MMI_ERR_HIP, "out of pinned host memory (TTS script staging)");
            }
            lm->tts_stage_ev.assign(G, nullptr);
            lm->tts_stage_used.assign(G, 0);
            for (int i = 0; i < G; ++i) MMI_HIP_CHECK(hipEventCreateWithFlags(&lm->tts_stage_ev[i], hipEventDisableTiming));
        }
        int rc = 0;
        if (lm->xkv) {      // the cross source projection: all rows at once, or row by row into a capacity above the start's length
            const uint16_t* src = reinterpret_cast<const uint16_t*>(guide->condition_cross);
            if (lm->cross_cap == lm->cross_len) rc = project_cross_source(lm, src, 0, B * lm->cross_len, s);
            for (int r = 0; lm->cross_cap != lm->cross_len && r < B && !rc; ++r)
                rc = project_cross_source(lm, src + (size_t)r * lm->cross_len * d, (size_t)r * lm->cross_cap, lm->cross_len, s);
        }
        if (!rc && lm->lp_on) rc = logprobs_alloc(lm, s);
        if (!rc) rc = build_program(lm);
        if (!rc && lm->prefill_rows > 0) rc = prefill_alloc(lm, s);
        if (rc) return rc;
        MMI_HIP_CHECK(hipStreamSynchronize(s));
        return MMI_OK;
    };
    if ((rc = rest())) return fail(rc);
    if (lm->knobs.debug_trace) {
        static int session = 0;
        lm->trace_name = lm->knobs.debug_trace_prefix + "." + std::to_string(session++);
        lm->trace_file = fopen(lm->trace_name.c_str(), "w");
        lm->trace_prev.assign(lm->st.ptrs.size(), 0ull);
        lm->trace_step = 0;
        if (lm->trace_file && hipMalloc((void**)&lm->trace_dev, lm->st.ptrs.size() * sizeof(unsigned long long)) != hipSuccess) {
            fclose(lm->trace_file);
            lm->trace_file = nullptr;
        }
    }
    lm->streaming = true;
    return MMI_OK;
}

extern "C" int mmi_lm_streaming_stop(mmi_lm* lm) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming) return MMI_OK;
    hipDeviceSynchronize();
    if (lm->trace_file) { fclose(lm->trace_file); lm->trace_file = nullptr; }
    if (lm->trace_dev) { hipFree(lm->trace_dev); lm->trace_dev = nullptr; }
    lm->prog.clear();
    lm->st.release();
    lm->pf_mem.release();
    lm->lp_mem.release();
    lm->lp = LpRings{nullptr, nullptr, nullptr, 0, 0};
    for (BufTable* t : {&lm->st_table, &lm->pf_table}) {      // no member keeps pointing into the freed arenas
        for (BufDecl& e : *t) *e.slot = nullptr;
        t->clear();
    }
    lm->offsets_m = nullptr;                                  // (the alias of `offsets` on a stream without guidance)
    lm->row_slot_h.clear();
    lm->row_top_p.clear();
    lm->nucleus_live = false;
    if (lm->tts_stage) { hipHostFree(lm->tts_stage); lm->tts_stage = nullptr; }
    for (hipEvent_t e : lm->tts_stage_ev) if (e) hipEventDestroy(e);
    lm->tts_stage_ev.clear();
    lm->tts_stage_used.clear();
    lm->streaming = false;
    lm->batch = 0;
    lm->gen_batch = 0;
    lm->cfg_coef = 1.f;
    return MMI_OK;
}

extern "C" int mmi_lm_set_exec_mask(mmi_lm* lm, const uint8_t* mask, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !mask) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    MMI_HIP_CHECK(hipMemcpyAsync(lm->exec, mask, lm->gen_batch, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MMI_OK;
}

extern "C" int mmi_lm_reset(mmi_lm* lm, const uint8_t* mask, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    TokArgs t = tok_args(lm);
    MMI_LAUNCH(k_lm_reset, mmi_cdiv(lm->gen_batch, 64), 64, 0, (hipStream_t)stream, t, mask, lm->exec);
    MMI_CHECK_LAUNCH();
    const int rc = clear_logprobs(lm, (hipStream_t)stream, mask);
    if (rc) return rc;
    lm->offset_cpu = 0;   // lm.py:540: any reset, even partial, zeroes the host-side step counter
    return MMI_OK;
}

// ---- forking a session ---------------------------------------------------------------------------------------
// No reference counterpart (the nearest: get_streaming_state / set_streaming_state on a batch of one, streaming.py:158-181).
// Stream-ordered: two launches (the ring, the per-session rows) and the clearing of the destinations' log-probability rings; the
// ring's valid length is read on the device, its grid sized by depth_bound.  What a session is comes from state_table(): every
// entry with per-session slices except the ring (k_fork_ring) and `exec` (set to 1), plus the per-layer slices of `xkv` and the
// nucleus tail behind `rowtab`.
extern "C" int mmi_lm_fork_session(mmi_lm* lm, int32_t src, const int32_t* dst, int32_t n_dst, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    const int G = lm->gen_batch, B = lm->batch;
    ForkSessions fs;
    int rc = mmi_fork_sessions("mmi_lm_fork_session", G, src, dst, n_dst, &fs);
    if (rc) return rc;
    fs.n_rows = B > G ? 2 : 1;
    fs.twin = G;
    hipStream_t s = (hipStream_t)stream;
    const mmi_lm_cfg& c = lm->cfg;
    const KvRing& ring = lm->ring;
    const int H = c.num_heads, Dh = c.dim / H;
    ForkRingArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.base[0] = reinterpret_cast<uint8_t*>(lm->kc); ra.base[1] = reinterpret_cast<uint8_t*>(lm->vc);
    ra.n_base = 2; ra.layers = c.num_layers; ra.layer_stride = (long)(ring.layer_u16 * sizeof(uint16_t));
    ra.n_planes = ring.form == 2 ? 2 : 1;
    ra.pos_bytes[0] = ring.form == 2 ? Dh / 2 : (ring.form == 1 ? Dh : 2 * Dh);
    ra.plane_off[1] = (long)ring.scale_off; ra.pos_bytes[1] = Dh / 16;
    ra.H = H; ra.cap = c.context; ra.s = fs;
    ra.len = lm->offsets;       // (not offsets_m: on a guided stream that is the last step's copy, one behind after the commit)
    for (int p = 0; p < ra.n_planes; ++p)
        ra.vec[p] = ((size_t)ra.layer_stride | (size_t)ra.plane_off[p] | ((size_t)ra.cap * ra.pos_bytes[p])) % 16 == 0 ? 1 : 0;
    ForkRowArgs rows;
    memset(&rows, 0, sizeof(rows));
    rows.exec = lm->exec; rows.s = fs;
    bool full = false;
    for (const BufDecl& e : lm->st_table) {
        const bool is_ring = e.slot == (void**)&lm->kc || e.slot == (void**)&lm->vc;
        if (e.slot == (void**)&lm->xkv) {         // [layers][B][cross_cap][2 * dim]: a slice per layer and model row
            const size_t slice = (size_t)lm->cross_cap * 2 * c.dim * e.elem;
            full = full || !mmi_fork_add(rows, *e.slot, c.num_layers, (size_t)B * slice, slice, slice, true);
        }
        if (e.rows <= 0 || is_ring || e.slot == (void**)&lm->exec) continue;
        const size_t slice = e.count * e.elem / (size_t)e.rows;
        full = full || !mmi_fork_add(rows, *e.slot, 1, 0, slice, slice, e.rows == B && B > G);
        if (e.tail && e.slot == (void**)&lm->rowtab)      // the sessions' nucleus values behind the row table
            full = full || !mmi_fork_add(rows, lm->rowtab + G, 1, 0, sizeof(RowTopP), sizeof(RowTopP), false);
    }
    if (full) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_fork_session: the state table outgrew the descriptor list");
    // depth_bound bounds the sessions' offsets - except on a guided stream restored from a snapshot: mmi_lm_state_load takes it from
    // offsets_m, which is one behind offsets there (k_lm_cfg_twins writes it at the head of a step), and every later step keeps
    // that distance.  One more position covers it; the valid length itself is read on the device
    if ((rc = mmi_launch_fork_ring(s, ra, lm->depth_bound + (B > G ? 1 : 0)))) return rc;
    if ((rc = mmi_launch_fork_rows(s, rows))) return rc;
    uint8_t sess[MMI_FORK_MAX_DST];
    for (int i = 0; i < n_dst; ++i) sess[i] = (uint8_t)dst[i];
    if ((rc = clear_logprobs(lm, s, nullptr, sess, n_dst))) return rc;
    // the host's mirrors of per-session device values (the ones mmi_lm_state_load refreshes)
    for (int i = 0; i < n_dst; ++i) {
        lm->row_active[dst[i]] = lm->row_active[src];
        if (lm->nucleus_live) lm->row_top_p[dst[i]] = lm->row_top_p[src];
        if (lm->row_slot) lm->row_slot_h[dst[i]] = lm->row_slot_h[src];
    }
    return MMI_OK;
}

// ---- per-session sampling ---------------------------------------------------------------------------------------------------
static int write_rows(mmi_lm* lm, const uint8_t* mask, const mmi_row_sampling* rows, hipStream_t s) {
    const int G = lm->gen_batch;
    RowSampSet set;
    memset(&set, 0, sizeof(set));
    auto flush = [&]() -> int {
        if (!set.n) return MMI_OK;
        MMI_LAUNCH(k_lm_set_rows, 1, 64, 0, s, lm->rowtab, set, G);
        MMI_CHECK_LAUNCH();
        set.n = 0;
        return MMI_OK;
    };
    for (int b = 0; b < G; ++b) {
        if (mask && !mask[b]) continue;
        RowSamp e;
        memset(&e, 0, sizeof(e));                       // active = 0, hist_n = 0: the handle's settings, an empty ring
        if (rows) {
            const mmi_row_sampling& r = rows[b];
            e.active = 1; e.use_sampling = r.use_sampling ? 1 : 0; e.top_k = r.top_k; e.top_k_text = r.top_k_text;
            e.temp = r.temp; e.temp_text = r.temp_text; e.pad_mult = r.pad_mult; e.rep_penalty = r.repetition_penalty;
            e.seed = r.seed; e.rep_context = r.repetition_context;
        }
        set.e[set.n] = e; set.row[set.n] = b;
        if (++set.n == 16) { int rc = flush(); if (rc) return rc; }
        lm->row_active[b] = rows ? 1 : 0;
    }
    return flush();
}

extern "C" int mmi_lm_set_row_sampling(mmi_lm* lm, const uint8_t* mask, const mmi_row_sampling* rows, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !rows) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    for (int b = 0; b < lm->gen_batch; ++b)            // all or nothing: a refused call changes no row
        if (!mask || mask[b]) { int rc = mmi_row_sampling_check(&rows[b]); if (rc) return rc; }
    return write_rows(lm, mask, rows, (hipStream_t)stream);
}

// ---- per-session conditions ---------------------------------------------------------------------------------------------------
extern "C" int mmi_lm_set_cross_capacity(mmi_lm* lm, int32_t positions) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "the capacity sizes the stream's keys / values buffer: set it before streaming_start");
    if (positions < 0) return mmi_fail(MMI_ERR_INVALID, "capacity must be >= 0 (0 = the start's cross_len)");
    lm->cross_cap_set = positions;
    return MMI_OK;
}

extern "C" int mmi_lm_cross_capacity(const mmi_lm* lm) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    return lm->streaming ? lm->cross_cap : lm->cross_cap_set;
}

extern "C" int mmi_lm_set_row_condition(mmi_lm* lm, int32_t session, const mmi_row_condition* c, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !c) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if (session < 0 || session >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "session outside [0, batch)");
    if (!std::isfinite(c->cfg_coef)) return mmi_fail(MMI_ERR_INVALID, "cfg_coef must be finite");
    const bool guided = lm->batch > lm->gen_batch;
    if (c->cfg_coef != 1.f && !guided)
        return mmi_fail(MMI_ERR_STATE, "cfg_coef != 1 needs a stream started with guidance (two model rows per session)");
    if (c->condition_sum && !lm->cond)
        return mmi_fail(MMI_ERR_STATE, "the stream was started without a sum condition: it has no buffer for one");
    if (c->condition_cross && !lm->cfg.cross_attention)
        return mmi_fail(MMI_ERR_INVALID, "a cross-attention condition was given to a model without cross-attention layers");
    if (c->condition_cross && (c->cross_len < 1 || c->cross_len > lm->cross_cap))
        return mmi_fail(MMI_ERR_SHAPE, "cross_len outside [1, capacity] (mmi_lm_set_cross_capacity)");
    hipStream_t s = (hipStream_t)stream;
    const int G = lm->gen_batch, d = lm->cfg.dim, R = guided ? 2 : 1;
    if (c->condition_cross) {       // the session's row(s): positions [0, cross_len) of their own slots; nothing else is touched
        const uint16_t* src = reinterpret_cast<const uint16_t*>(c->condition_cross);
        const long counted = lm->xlds_launches;       // mmi_lm_stat(lm, 0) counts the step's launches, not these
        for (int r = 0; r < R; ++r) {
            int rc = project_cross_source(lm, src + (size_t)r * c->cross_len * d, (size_t)(r * G + session) * lm->cross_cap, c->cross_len, s);
            if (rc) return rc;
        }
        lm->xlds_launches = counted;
    }
    RowCondSet set;
    memset(&set, 0, sizeof(set));
    set.session = session; set.G = G; set.rows = R; set.len = c->condition_cross ? c->cross_len : 0; set.coef = c->cfg_coef;
    set.sum = reinterpret_cast<const uint16_t*>(c->condition_sum); set.D = d;
    MMI_LAUNCH(k_lm_set_row_cond, mmi_cdiv(c->condition_sum ? d : 1, 256), 256, 0, s, lm->xlen, lm->coefs, lm->cond, set);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

// ---- per-row LoRA adapters (modules/lora.py, loaders.py:486-516) --------------------------------------------------
extern "C" int mmi_lm_enable_adapters(mmi_lm* lm, int32_t max_adapters, int32_t max_rank) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters add launches to the step's launch list: enable them before streaming_start");
    if (max_adapters == 0 && max_rank == 0) {
        lm->lora_on = false;
        lm->lora_S = lm->lora_R = 0;
        lm->lora_by_wp.clear();
        lm->lora_by_name.clear();
        lm->lora_mem.release();
        lm->lora_bad = nullptr;
        return MMI_OK;
    }
    if (max_adapters < 1 || max_adapters > 8) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_enable_adapters: max_adapters must be 1..8");
    if (max_rank != 32 && max_rank != 64 && max_rank != 96 && max_rank != 128)
        return mmi_fail(MMI_ERR_INVALID, "mmi_lm_enable_adapters: max_rank must be 32, 64, 96 or 128 (whole k-steps at both tiles)");
    if (lm->lora_on) return mmi_fail(MMI_ERR_STATE, "mmi_lm_enable_adapters: already enabled (turn them off with (0, 0) first)");
    const mmi_lm_cfg& c = lm->cfg;
    if (lm->q8 > 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters on quantised linears (int8 / fp8 / MXFP4) are not supported: the tail runs on the bf16 MFMA of a bf16 linear");
    if (lm->max_batch > 64) return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters are not supported above 64 model rows (k_gemm_rows has no adapter tail)");
    if (c.cross_attention) return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters are not supported on models with cross-attention layers");
    if (c.extra_heads_num_heads > 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters are not supported on models with extra heads (the reference wraps their linears too)");
    if (lm->demux || lm->text_emb2 || lm->vector_by_name.count("depformer_text_emb.low_rank.weight"))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters are not supported with low-rank or demuxed embeddings (the reference wraps their linears too)");
    if (lm->Td != lm->T) return mmi_fail(MMI_ERR_UNSUPPORTED, "adapters are not supported with the depth transformer on its own tile (MMI_DEP_TILE)");
    const int S = max_adapters, R = max_rank, SR = S * R;
    auto fail = [&](int code) { lm->lora_by_wp.clear(); lm->lora_by_name.clear(); lm->lora_mem.release(); lm->lora_bad = nullptr; return code; };
    lm->lora_mem.poison = 0;
    for (const auto& kv : lm->linear_by_name) {
        const GemmW& g = kv.second;
        if (lm->lora_by_wp.count(g.wp)) { lm->lora_by_name[kv.first] = g.wp; continue; }
        LoraBank bk;
        const size_t na = (size_t)(SR / g.T) * g.KSTEPS * 64, nb = (size_t)g.NT * (SR / mmi_kstep(g.T)) * 64;     // 16-byte entries
        if (lm->lora_mem.alloc(&bk.a, na) != hipSuccess || lm->lora_mem.alloc(&bk.b, nb) != hipSuccess)
            return fail(mmi_fail(MMI_ERR_HIP, "out of device memory (adapter banks)"));
        if (hipMemset(bk.a, 0, na * 16) != hipSuccess || hipMemset(bk.b, 0, nb * 16) != hipSuccess) return fail(mmi_fail(MMI_ERR_HIP, "memset"));
        lm->lora_by_wp[g.wp] = bk;
        lm->lora_by_name[kv.first] = g.wp;
    }
    if (lm->lora_mem.alloc(&lm->lora_bad, (size_t)1) != hipSuccess) return fail(mmi_fail(MMI_ERR_HIP, "out of device memory (adapter banks)"));
    lm->lora_S = S; lm->lora_R = R;
    lm->lora_on = true;
    return MMI_OK;
}

namespace {
const GemmW* lora_linear(const mmi_lm* lm, const std::string& weight_name) {
    auto it = lm->linear_by_name.find(weight_name);
    return it == lm->linear_by_name.end() ? nullptr : &it->second;
}
int lora_slot_free(const mmi_lm* lm, int slot, const char* what) {
    if (!lm->lora_on) return mmi_fail(MMI_ERR_STATE, std::string(what) + ": the handle has no adapters (mmi_lm_enable_adapters)");
    if (slot < 0 || slot >= lm->lora_S) return mmi_fail(MMI_ERR_INVALID, std::string(what) + ": slot outside [0, max_adapters)");
    if (lm->streaming)
        for (int v : lm->row_slot_h)
            if (v == slot) return mmi_fail(MMI_ERR_STATE, std::string(what) + ": a live session runs on this slot");
    return MMI_OK;
}
// slot `slot` of every bank zeroed (stream ordered)
int lora_zero_slot(mmi_lm* lm, int slot, hipStream_t s) {
    const int R = lm->lora_R, SR = lm->lora_S * R;
    for (const auto& kv : lm->linear_by_name) {
        const GemmW& g = kv.second;
        const LoraBank& bk = lm->lora_by_wp[g.wp];
        const size_t na = (size_t)(R / g.T) * g.KSTEPS * 64;
        MMI_HIP_CHECK(hipMemsetAsync(bk.a + (size_t)slot * na, 0, na * 16, s));
        const int ksr = R / mmi_kstep(g.T);
        const long n = (long)g.NT * ksr * 512;
        MMI_LAUNCH(k_pack_lora_slot, (int)mmi_cdiv64((int64_t)n, 256), 256, 0, s, (const uint16_t*)nullptr, reinterpret_cast<uint16_t*>(bk.b), 0, 0,
                   g.T, g.NT, ksr, 0, SR / mmi_kstep(g.T), slot * ksr, 1.f);
    }
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}
}  // namespace

extern "C" int mmi_lm_load_adapter(mmi_lm* lm, int32_t slot, float scaling, const mmi_tensor_desc* descs, int32_t n, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || (!descs && n > 0) || n < 0) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_load_adapter: bad argument");
    int rc = lora_slot_free(lm, slot, "mmi_lm_load_adapter");
    if (rc) return rc;
    if (!std::isfinite(scaling)) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_load_adapter: scaling must be finite");
    hipStream_t s = (hipStream_t)stream;
    const int R = lm->lora_R, SR = lm->lora_S * R;
    // ---- every check before anything is written
    struct Pair { const mmi_tensor_desc* a = nullptr; const mmi_tensor_desc* b = nullptr; };
    std::map<std::string, Pair> pairs;          // by `<linear>.weight`
    const std::string sa = ".lora_A.weight", sb = ".lora_B.weight", sf = ".frozen_W.weight";
    auto ends = [](const std::string& k, const std::string& suf) { return k.size() > suf.size() && k.compare(k.size() - suf.size(), suf.size(), suf) == 0; };
    for (int i = 0; i < n; ++i) {
        const std::string key = descs[i].name ? descs[i].name : "";
        if (ends(key, sf)) continue;             // (the base weight under the name a LoRALinear gives it: not the adapter's)
        const bool isa = ends(key, sa), isb = ends(key, sb);
        const std::string stem = (isa || isb) ? key.substr(0, key.size() - sa.size()) : key;
        if ((!isa && !isb) || !lora_linear(lm, stem + ".weight"))
            return mmi_fail(MMI_ERR_INVALID, "unexpected_keys in the lora weights: " + key);          // loaders.py:508-511
        if (descs[i].dtype != MMI_BF16 || descs[i].ndim != 2 || !descs[i].data) return mmi_fail(MMI_ERR_INVALID, "adapter tensors must be bf16 matrices: " + key);
        (isa ? pairs[stem + ".weight"].a : pairs[stem + ".weight"].b) = &descs[i];
    }
    for (const auto& kv : pairs) {
        const GemmW& g = *lora_linear(lm, kv.first);
        const std::string stem = kv.first.substr(0, kv.first.size() - 7);
        if (!kv.second.a || !kv.second.b) return mmi_fail(MMI_ERR_INVALID, "LoRA weights carry " + stem + (kv.second.a ? sa + " without " + stem + sb : sb + " without " + stem + sa));
        const mmi_tensor_desc &A = *kv.second.a, &Bm = *kv.second.b;
        const long r = A.shape[0], Nfull = g.gate ? 2L * g.N : g.N;
        if (r < 8 || r % 8 != 0 || r > R) return mmi_fail(MMI_ERR_INVALID, "adapter rank must be a multiple of 8 and at most max_rank: " + stem);
        if (A.shape[1] != g.K || Bm.shape[0] != Nfull || Bm.shape[1] != r) return mmi_fail(MMI_ERR_INVALID, "LoRA shapes do not fit " + kv.first);
    }
    MMI_HIP_CHECK(hipMemsetAsync(lm->lora_bad, 0, sizeof(int), s));
    for (const auto& kv : pairs) {
        const mmi_tensor_desc &A = *kv.second.a, &Bm = *kv.second.b;
        const long na = (long)A.shape[0] * A.shape[1], nb = (long)Bm.shape[0] * Bm.shape[1];
        MMI_LAUNCH(k_lora_check_finite, (int)mmi_cdiv64(na, 256), 256, 0, s, (const uint16_t*)A.data, na, 1.f, lm->lora_bad);
        MMI_LAUNCH(k_lora_check_finite, (int)mmi_cdiv64(nb, 256), 256, 0, s, (const uint16_t*)Bm.data, nb, scaling, lm->lora_bad);
    }
    MMI_CHECK_LAUNCH();
    int bad = 0;
    MMI_HIP_CHECK(hipMemcpyAsync(&bad, lm->lora_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    MMI_HIP_CHECK(hipStreamSynchronize(s));
    if (bad) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_load_adapter: the adapter (or scaling * lora_B in bf16) holds values that are not finite");
    // ---- the slot: zero everywhere, then the linears the adapter mentions
    if ((rc = lora_zero_slot(lm, slot, s))) return rc;
    for (const auto& kv : pairs) {
        const GemmW& g = *lora_linear(lm, kv.first);
        const LoraBank& bk = lm->lora_by_wp[g.wp];
        const mmi_tensor_desc &A = *kv.second.a, &Bm = *kv.second.b;
        const int r = (int)A.shape[0], ksr = R / mmi_kstep(g.T);
        const size_t na = (size_t)(R / g.T) * g.KSTEPS * 64;
        const long ea = (long)(R / g.T) * g.KSTEPS * 512, eb = (long)g.NT * ksr * 512;
        MMI_LAUNCH(k_pack_lora_slot, (int)mmi_cdiv64((int64_t)ea, 256), 256, 0, s, (const uint16_t*)A.data, reinterpret_cast<uint16_t*>(bk.a + (size_t)slot * na),
                   r, g.K, g.T, R / g.T, g.KSTEPS, 0, g.KSTEPS, 0, 1.f);
        MMI_LAUNCH(k_pack_lora_slot, (int)mmi_cdiv64((int64_t)eb, 256), 256, 0, s, (const uint16_t*)Bm.data, reinterpret_cast<uint16_t*>(bk.b),
                   (int)Bm.shape[0], r, g.T, g.NT, ksr, g.gate ? g.N : 0, SR / mmi_kstep(g.T), slot * ksr, scaling);
    }
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

extern "C" int mmi_lm_unload_adapter(mmi_lm* lm, int32_t slot, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    int rc = lora_slot_free(lm, slot, "mmi_lm_unload_adapter");
    if (rc) return rc;
    return lora_zero_slot(lm, slot, (hipStream_t)stream);
}

extern "C" int mmi_lm_set_row_adapter(mmi_lm* lm, int32_t session, int32_t slot, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming || !lm->row_slot) return mmi_fail(MMI_ERR_STATE, "adapters are not enabled on a live stream (mmi_lm_enable_adapters, then streaming_start)");
    if (session < 0 || session >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "session outside [0, batch)");
    if (slot < -1 || slot >= lm->lora_S) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_set_row_adapter: slot must be -1 (none) or in [0, max_adapters)");
    MMI_LAUNCH(k_fill_i32, 1, 64, 0, (hipStream_t)stream, lm->row_slot + session, (int)slot, 1L);
    MMI_CHECK_LAUNCH();
    lm->row_slot_h[session] = slot;
    return MMI_OK;
}

int mmi_lm_adapter_slots(const mmi_lm* lm) { return lm && lm->lora_on ? lm->lora_S : 0; }      // (batcher.hip)

extern "C" int32_t mmi_lm_row_adapter(const mmi_lm* lm, int32_t session) {
    if (!lm || !lm->streaming || !lm->row_slot || session < 0 || session >= lm->gen_batch) return -1;
    return lm->row_slot_h[session];
}

// ---- the TTS script machine ---------------------------------------------------------------------------------------------------
extern "C" int mmi_lm_enable_tts_machine(mmi_lm* lm, const mmi_tts_params* p, int32_t max_entries, int32_t max_tokens, int32_t max_prefix) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "the machine adds ops to the step's launch list: enable it before streaming_start");
    if (!p) { lm->tts_on = false; return MMI_OK; }
    const mmi_lm_cfg& c = lm->cfg;
    if (c.dep_q == 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "the TTS machine feeds the depth transformer: the model has dep_q == 0");
    if (p->second_stream_ahead > 0 && !lm->demux)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "second_stream_ahead > 0 needs a model with a demuxed text stream");
    if (max_entries < 0 || max_tokens < 0 || max_prefix < 0 || p->second_stream_ahead < 0 || p->max_padding < 0 || p->initial_padding < 0 ||
        p->delay_steps < 0 || !std::isfinite(p->padding_bonus))
        return mmi_fail(MMI_ERR_INVALID, "mmi_tts_params: negative capacity / count or a non-finite padding bonus");
    if (p->new_word < 0 || p->new_word > c.text_card || p->pad < 0 || p->pad > c.text_card || p->new_word == p->pad)
        return mmi_fail(MMI_ERR_INVALID, "mmi_tts_params: new_word and pad must be two ids of the text vocabulary");
    if (p->zero != -1) return mmi_fail(MMI_ERR_INVALID, "mmi_tts_params: zero must be -1, the token the embeddings map to a zero row");
    if (lm->demux && p->text_card != c.text_card + 1)
        return mmi_fail(MMI_ERR_INVALID, "mmi_tts_params: text_card (the mux base) must be the model's text_card + 1");
    if ((int64_t)2 * max_tokens + 3 * (int64_t)max_entries + (int64_t)(1 + c.dep_q) * max_prefix > (1 << 26))
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_enable_tts_machine: capacities above 2^26 words per session");
    lm->tts_p.text_card = p->text_card; lm->tts_p.new_word = p->new_word; lm->tts_p.pad = p->pad; lm->tts_p.zero = p->zero;
    lm->tts_p.second_stream_ahead = p->second_stream_ahead; lm->tts_p.max_padding = p->max_padding;
    lm->tts_p.initial_padding = p->initial_padding; lm->tts_p.delay_steps = p->delay_steps; lm->tts_p.padding_bonus = p->padding_bonus;
    lm->tts_max_entries = max_entries; lm->tts_max_tokens = max_tokens; lm->tts_max_prefix = max_prefix;
    lm->tts_on = true;
    return MMI_OK;
}

extern "C" int mmi_lm_set_row_script(mmi_lm* lm, int32_t session, const mmi_tts_script* sc, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming || !lm->tts) return mmi_fail(MMI_ERR_STATE, "the TTS machine is not enabled on a live stream (mmi_lm_enable_tts_machine, then streaming_start)");
    if (session < 0 || session >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "session outside [0, batch)");
    const mmi_lm_cfg& c = lm->cfg;
    const int me = lm->tts_max_entries, mt = lm->tts_max_tokens, mp = lm->tts_max_prefix;
    int ntok = 0;
    if (sc) {       // every check before the first write: a refused call changes nothing
        if (sc->n_entries < 0 || sc->text_prefix_len < 0 || sc->audio_prefix_len < 0) return mmi_fail(MMI_ERR_INVALID, "negative count in mmi_tts_script");
        if (sc->n_entries > me) return mmi_fail(MMI_ERR_SHAPE, "more script entries than the machine's capacity (max_entries)");
        if (sc->text_prefix_len > mp || sc->audio_prefix_len > mp) return mmi_fail(MMI_ERR_SHAPE, "more prefix columns than the machine's capacity (max_prefix)");
        if (sc->n_entries > 0 && (!sc->entry_first || !sc->entry_padding)) return mmi_fail(MMI_ERR_INVALID, "null entry arrays");
        if ((sc->text_prefix_len > 0 && !sc->text_prefix) || (sc->audio_prefix_len > 0 && !sc->audio_prefix)) return mmi_fail(MMI_ERR_INVALID, "null prefix array");
        if (sc->n_entries > 0) {
            if (sc->entry_first[0] != 0) return mmi_fail(MMI_ERR_INVALID, "entry_first[0] must be 0");
            for (int e = 0; e < sc->n_entries; ++e) {
                if (sc->entry_first[e + 1] < sc->entry_first[e]) return mmi_fail(MMI_ERR_INVALID, "entry_first must not decrease");
                if (sc->entry_padding[e] < 0) return mmi_fail(MMI_ERR_INVALID, "negative padding in a script entry");
            }
            ntok = sc->entry_first[sc->n_entries];
        }
        if (ntok > mt) return mmi_fail(MMI_ERR_SHAPE, "more script tokens than the machine's capacity (max_tokens)");
        if (ntok > 0 && !sc->tokens) return mmi_fail(MMI_ERR_INVALID, "null token array");
        for (int i = 0; i < ntok; ++i)
            if (sc->tokens[i] < 0 || sc->tokens[i] > c.text_card) return mmi_fail(MMI_ERR_INVALID, "a script token outside the text vocabulary");
        const int64_t N = (int64_t)c.text_card + 1, top = lm->demux ? N * (N + 1) : N;        // a prefix token may be a muxed pair, or `zero`
        for (int i = 0; i < sc->text_prefix_len; ++i)
            if (sc->text_prefix[i] < -1 || sc->text_prefix[i] >= top) return mmi_fail(MMI_ERR_INVALID, "a text prefix token outside the text vocabulary");
        for (int i = 0; i < c.dep_q * sc->audio_prefix_len; ++i)
            if (sc->audio_prefix[i] < -2 || sc->audio_prefix[i] >= c.card) return mmi_fail(MMI_ERR_INVALID, "an audio prefix token outside the codebook");
    }
    hipStream_t s = (hipStream_t)stream;
    // the session's own pinned row; the copy out of it of an earlier call has normally long completed (no wait in that case)
    if (lm->tts_stage_used[session]) MMI_HIP_CHECK(hipEventSynchronize(lm->tts_stage_ev[session]));
    int* r = lm->tts_stage + (size_t)session * lm->tts_stride;
    memset(r, 0, (size_t)lm->tts_stride * sizeof(int));
    r[MMI_TTS_REMAIN] = r[MMI_TTS_FORCED] = lm->tts_p.initial_padding;        // new_state (tts.py:151-158)
    r[MMI_TTS_END] = -1;
    if (sc) {
        r[MMI_TTS_HAS] = 1; r[MMI_TTS_NENT] = sc->n_entries; r[MMI_TTS_TPLEN] = sc->text_prefix_len; r[MMI_TTS_APLEN] = sc->audio_prefix_len;
        int* q = r + MMI_TTS_HDR;
        for (int i = 0; i < ntok; ++i) q[i] = sc->tokens[i];
        q += mt;
        for (int e = 0; e <= sc->n_entries && sc->n_entries > 0; ++e) q[e] = sc->entry_first[e];
        q += me + 1;
        for (int e = 0; e < sc->n_entries; ++e) q[e] = sc->entry_padding[e];
        q += 2 * me + mt;       // past consumption_times and the lookahead buffer
        for (int i = 0; i < sc->text_prefix_len; ++i) q[i] = sc->text_prefix[i];
        q += mp;
        for (int k = 0; k < c.dep_q; ++k)
            for (int i = 0; i < sc->audio_prefix_len; ++i) q[k * mp + i] = sc->audio_prefix[(size_t)k * sc->audio_prefix_len + i];
    }
    MMI_HIP_CHECK(hipMemcpyAsync(lm->tts + (size_t)session * lm->tts_stride, r, (size_t)lm->tts_stride * sizeof(int), hipMemcpyHostToDevice, s));
    MMI_HIP_CHECK(hipEventRecord(lm->tts_stage_ev[session], s));
    lm->tts_stage_used[session] = 1;
    return MMI_OK;
}

extern "C" int mmi_lm_row_script_status(mmi_lm* lm, int32_t session, mmi_tts_status* out, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !out) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming || !lm->tts) return mmi_fail(MMI_ERR_STATE, "the TTS machine is not enabled on a live stream");
    if (session < 0 || session >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "session outside [0, batch)");
    hipStream_t s = (hipStream_t)stream;
    const int me = lm->tts_max_entries, mt = lm->tts_max_tokens;
    const int* r = lm->tts + (size_t)session * lm->tts_stride;
    int hdr[MMI_TTS_HDR];
    std::vector<int> times((size_t)me);
    MMI_HIP_CHECK(hipMemcpyAsync(hdr, r, sizeof(hdr), hipMemcpyDeviceToHost, s));
    if (me > 0) MMI_HIP_CHECK(hipMemcpyAsync(times.data(), r + MMI_TTS_HDR + mt + 2 * me + 1, (size_t)me * sizeof(int), hipMemcpyDeviceToHost, s));
    MMI_HIP_CHECK(hipStreamSynchronize(s));      // a status read returns host values: it waits for the steps enqueued so far
    out->has_script = hdr[MMI_TTS_HAS];
    out->end_step = hdr[MMI_TTS_HAS] ? hdr[MMI_TTS_END] : -1;       // a row without a script never ends (its words are all 0 after the start)
    out->n_consumed = hdr[MMI_TTS_HAS] ? hdr[MMI_TTS_NCONS] : 0;
    if (out->consumption_times)
        for (int i = 0; i < hdr[MMI_TTS_NCONS] && i < out->capacity; ++i) out->consumption_times[i] = times[(size_t)i];
    return MMI_OK;
}

extern "C" int mmi_lm_set_text_end_padding_id(mmi_lm* lm, int32_t id) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "the end-of-padding id is part of the step's launch list: set it before streaming_start");
    if (id < 0 || id > lm->cfg.text_card) return mmi_fail(MMI_ERR_INVALID, "end-of-padding id outside the text vocabulary");
    lm->text_eop = id;
    return MMI_OK;
}

// ---- nucleus (top-p) sampling, DESIGN.md 8.17 ---------------------------------------------------------------------------------
static int top_p_check(float top_p, float top_p_text) {
    for (float v : {top_p, top_p_text})
        if (!std::isfinite(v) || v < 0.f || v > 1.f) return mmi_fail(MMI_ERR_INVALID, "top_p and top_p_text must lie in [0, 1] (0 = off)");
    return MMI_OK;
}

extern "C" int mmi_lm_enable_nucleus(mmi_lm* lm, int32_t on) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "the nucleus samplers are part of the step's launch list: enable them before streaming_start");
    if (!on && (lm->top_p > 0.f || lm->top_p_text > 0.f))
        return mmi_fail(MMI_ERR_STATE, "the handle's top_p is positive: set it to 0 (mmi_lm_set_top_p) before disabling the nucleus samplers");
    lm->nucleus_on = on != 0;
    return MMI_OK;
}

extern "C" int mmi_lm_set_top_p(mmi_lm* lm, float top_p, float top_p_text) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "the handle's top_p applies from streaming_start: set it before (a live session: mmi_lm_set_row_top_p)");
    int rc = top_p_check(top_p, top_p_text);
    if (rc) return rc;
    if ((top_p > 0.f || top_p_text > 0.f) && !lm->nucleus_on)
        return mmi_fail(MMI_ERR_STATE, "top_p > 0 needs the nucleus samplers (mmi_lm_enable_nucleus)");
    lm->top_p = top_p;
    lm->top_p_text = top_p_text;
    return MMI_OK;
}

extern "C" int mmi_lm_top_p(const mmi_lm* lm, float* top_p, float* top_p_text) {
    if (!lm || !top_p || !top_p_text) return mmi_fail(MMI_ERR_INVALID, "null argument");
    *top_p = lm->top_p;
    *top_p_text = lm->top_p_text;
    return MMI_OK;
}

extern "C" int32_t mmi_lm_nucleus_enabled(const mmi_lm* lm) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    return (lm->streaming ? lm->nucleus_live : lm->nucleus_on) ? 1 : 0;
}

static int write_row_top_p(mmi_lm* lm, int32_t session, RowTopP v, hipStream_t s) {
    MMI_LAUNCH(k_lm_set_row_top_p, 1, 64, 0, s, lm->rowtab, lm->gen_batch, (int)session, v.top_p, v.top_p_text);
    MMI_CHECK_LAUNCH();
    lm->row_top_p[session] = v;
    return MMI_OK;
}

extern "C" int mmi_lm_set_row_top_p(mmi_lm* lm, int32_t session, float top_p, float top_p_text, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if (!lm->nucleus_live) return mmi_fail(MMI_ERR_STATE, "the stream was started without the nucleus samplers (mmi_lm_enable_nucleus before streaming_start)");
    if (session < 0 || session >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "session outside [0, batch)");
    int rc = top_p_check(top_p, top_p_text);
    if (rc) return rc;
    return write_row_top_p(lm, session, RowTopP{top_p, top_p_text}, (hipStream_t)stream);
}

extern "C" int mmi_lm_clear_row_top_p(mmi_lm* lm, int32_t session, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if (!lm->nucleus_live) return mmi_fail(MMI_ERR_STATE, "the stream was started without the nucleus samplers (mmi_lm_enable_nucleus before streaming_start)");
    if (session < 0 || session >= lm->gen_batch) return mmi_fail(MMI_ERR_INVALID, "session outside [0, batch)");
    return write_row_top_p(lm, session, RowTopP{lm->top_p, lm->top_p_text}, (hipStream_t)stream);
}

extern "C" int mmi_lm_clear_row_sampling(mmi_lm* lm, const uint8_t* mask, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    return write_rows(lm, mask, nullptr, (hipStream_t)stream);
}

extern "C" int mmi_lm_step(mmi_lm* lm, const int64_t* user_codes, int32_t n_user, int64_t* out_tokens, float* opt_text_logits,
                           float* opt_audio_logits, const float* opt_noise, int32_t batch, int32_t* valid, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !out_tokens) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming)
        return mmi_fail(MMI_ERR_STATE, "You should wrap those calls with a `with lm_gen.streaming(): ...`.");   // lm.py:673-676
    if (!user_codes && lm->cfg.n_q > lm->cfg.dep_q) return mmi_fail(MMI_ERR_INVALID, "null argument");   // n_q == dep_q (TTS): no user stream
    if (batch != lm->gen_batch) return mmi_fail(MMI_ERR_SHAPE, "Got a different batch size than the streaming batch");   // lm.py:681
    const mmi_lm_cfg& c = lm->cfg;
    const int need_user = c.n_q - c.dep_q;
    if (n_user < need_user) return mmi_fail(MMI_ERR_SHAPE, "not enough user tokens");   // lm.py:683-686
    hipStream_t s = (hipStream_t)stream;
    const int B = batch;
    // refusals first: a refused step enqueues nothing
    if (opt_noise)
        for (uint8_t on : lm->row_active)
            if (on) return mmi_fail(MMI_ERR_UNSUPPORTED, "supplied noise is a parity aid of the handle's own sampling settings: not available while a session has settings of its own (mmi_lm_set_row_sampling)");
    if (opt_noise)
        for (const RowTopP& t : lm->row_top_p)
            if (t.top_p > 0.f || t.top_p_text > 0.f) return mmi_fail(MMI_ERR_UNSUPPORTED, "supplied noise is indexed by rank in the top-k: not available while a top_p is positive (mmi_lm_set_top_p, mmi_lm_set_row_top_p)");
    if (opt_noise && lm->samp.use_sampling && (lm->samp.top_k == 0 || lm->samp.top_k_text == 0))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "supplied noise is indexed by rank in the top-k: not available with top_k = 0");
    if (need_user > 0)
        MMI_LAUNCH(k_i64_to_i32, mmi_cdiv(B * need_user, 256), 256, 0, s, (const long*)user_codes, (long)n_user, lm->user_i32, B, need_user);
    if (opt_noise) {
        MMI_HIP_CHECK(hipMemcpyAsync(lm->noise, opt_noise, (size_t)B * (1 + c.dep_q) * lm->kmax * sizeof(float), hipMemcpyDeviceToDevice, s));
        MMI_HIP_CHECK(hipMemsetAsync(lm->use_noise, 1, 1, s));
        lm->noise_on = true;
    } else if (lm->noise_on) {          // the device flag only changes when the caller starts / stops supplying noise: no fill per step
        MMI_HIP_CHECK(hipMemsetAsync(lm->use_noise, 0, sizeof(int), s));
        lm->noise_on = false;
    }
    MMI_CHECK_LAUNCH();
    int rc;
    lm->prog.variant = attn_variant(lm, lm->attn_ns);
    const bool hooked = lm->hooks.on_text_logits || lm->hooks.on_text_token || lm->hooks.on_audio_tokens;
    if (hooked) {
        rc = run_step_with_hooks(lm, s);
        if (rc) {           // a hook aborted the step half-way: it is NOT committed (ring, offsets unchanged), and the forcing armed for
            hipMemsetAsync(lm->use_forced, 0, sizeof(int), s);   // this step does not leak into the next one
            lm->forced_armed = false;
        }
    }
    else if (lm->trace_file) {
        lm->prog.tap = [lm](size_t i, bool begin, hipStream_t st) {
            if (begin) return;
            const size_t n = lm->st.ptrs.size();
            hipMemsetAsync(lm->trace_dev, 0, n * sizeof(unsigned long long), st);
            for (size_t a = 0; a < n; ++a) {
                const long nb = (long)lm->st.sizes[a];
                int blocks = (int)((nb / 4 + 255) / 256);
                if (blocks > 2048) blocks = 2048;
                if (blocks < 1) blocks = 1;
                hipLaunchKernelGGL(k_checksum, blocks, 256, 0, st, (const uint8_t*)lm->st.ptrs[a], nb, lm->trace_dev + a);
            }
            std::vector<unsigned long long> now(n);
            hipStreamSynchronize(st);
            hipMemcpy(now.data(), lm->trace_dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            for (size_t a = 0; a < n; ++a)
                if (now[a] != lm->trace_prev[a])
                    fprintf(lm->trace_file, "%ld %zu %s %zu %zu %016llx\n", lm->trace_step, i, lm->prog.sites[i].c_str(), a, lm->st.sizes[a], now[a]);
            lm->trace_prev = now;
            // knobs.debug_dump = "step:op:alloc[,alloc...]": those allocations, as they are after that op, to <prefix>.<session>.a<alloc>
            if (const char* dd = lm->knobs.debug_dump.empty() ? nullptr : lm->knobs.debug_dump.c_str()) {
                long ds = -1, dop = -1;
                int used = 0;
                if (sscanf(dd, "%ld:%ld:%n", &ds, &dop, &used) >= 2 && ds == lm->trace_step && dop == (long)i) {
                    const char* q = dd + used;
                    while (*q) {
                        const long a = strtol(q, (char**)&q, 10);
                        if (*q == ',') ++q;
                        if (a < 0 || a >= (long)n) break;
                        std::vector<char> host(lm->st.sizes[a]);
                        hipMemcpy(host.data(), lm->st.ptrs[a], host.size(), hipMemcpyDeviceToHost);
                        if (FILE* df = fopen((lm->trace_name + ".a" + std::to_string(a)).c_str(), "wb")) { fwrite(host.data(), 1, host.size(), df); fclose(df); }
                    }
                }
            }
        };
        rc = lm->prog.run_eager(s);
        lm->prog.tap = nullptr;
        lm->trace_step += 1;
    }
    else if (lm->phase_fn) {
        auto fn = lm->phase_fn; void* user = lm->phase_user;
        rc = lm->prog.run_split(s, lm->use_graph && !lm->profiling, lm->cap_stream, lm->op_depformer, [fn, user](hipStream_t st) {
            return fn(user, (mmi_stream)st) ? mmi_fail(MMI_ERR_INVALID, "the phase callback reported an error") : (int)MMI_OK;
        });
    } else rc = lm->prog.run(s, lm->use_graph && !lm->profiling, lm->cap_stream);
    if (rc) return rc;
    if (lm->attn_ns > 1 && lm->use_graph && !lm->profiling && !hooked && attn_wave_kernel(lm->knobs) && !lm->knobs.no_precapture) {
        // both attention programs exist from the stream's first step on: the switch at depth solo_rows is then a graph launch
        // like any other (without this the deep program was captured + instantiated ~61 s into a live single-session stream)
        // The step above is already committed: a failure to capture the OTHER program (out of memory at instantiate, ...) must not
        // turn it into a failed call - the program is then captured when first needed, as before round 5.  The capture
        // re-runs every op closure: its GEMMs are not launches of this stream (mmi_lm_stat 0).
        const bool split = lm->phase_fn != nullptr;
        const long counted = lm->xlds_launches;
        for (int v = 0; v < MmiProgram::NV && !lm->precapture_failed; ++v)
            if (!lm->prog.ready(v, split) && lm->prog.precapture(v, lm->cap_stream, split, lm->op_depformer) != MMI_OK) {
                lm->precapture_failed = true;
                (void)hipGetLastError();
                fprintf(stderr, "moshi_mi: the second attention step program could not be captured ahead of time (%s); it will be captured when first needed\n",
                        mmi_last_error());
            }
        lm->xlds_launches = counted;
    }
    MMI_LAUNCH(k_i32_to_i64, mmi_cdiv(B * (c.dep_q + 1), 256), 256, 0, s, (const int*)lm->out_i32, (long*)out_tokens, B * (c.dep_q + 1));
    if (opt_text_logits)
        MMI_LAUNCH(k_bf16_to_f32, (int)mmi_cdiv64((int64_t)B * c.text_card_out, 256), 256, 0, s, (const uint16_t*)lm->text_logits, opt_text_logits, (long)B * c.text_card_out);
    if (opt_audio_logits) {
        // internal layout [dep_q][B][card] -> caller's [B][dep_q][card]
        for (int k = 0; k < c.dep_q; ++k)
            for (int b = 0; b < B; ++b)
                MMI_LAUNCH(k_bf16_to_f32, mmi_cdiv(c.card, 256), 256, 0, s, (const uint16_t*)(lm->dlogits + ((size_t)k * lm->batch + b) * c.card),
                           opt_audio_logits + ((size_t)b * c.dep_q + k) * c.card, (long)c.card);
    }
    MMI_CHECK_LAUNCH();
    if (lm->forced_armed) {   // forcing applies to one step only
        MMI_HIP_CHECK(hipMemsetAsync(lm->use_forced, 0, sizeof(int), s));
        lm->forced_armed = false;
    }
    lm->offset_cpu += 1;
    if (lm->depth_bound < (1L << 40)) lm->depth_bound += 1;
    if (valid) *valid = lm->offset_cpu > lm->max_delay ? 1 : 0;   // lm.py:774-776
    return MMI_OK;
}

extern "C" int mmi_lm_set_phase_callback(mmi_lm* lm, int (*fn)(void*, mmi_stream), void* user) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    lm->phase_fn = fn;
    lm->phase_user = user;
    return MMI_OK;
}

extern "C" int mmi_lm_set_hooks(mmi_lm* lm, const mmi_lm_hooks* hooks) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (hooks) lm->hooks = *hooks;
    else lm->hooks = mmi_lm_hooks{nullptr, nullptr, nullptr, nullptr};
    return MMI_OK;
}

extern "C" int mmi_lm_set_hidden_taps(mmi_lm* lm, int32_t on) {
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (lm->streaming) return mmi_fail(MMI_ERR_STATE, "mmi_lm_set_hidden_taps: call before streaming_start");
    lm->hidden_taps = on != 0;
    return MMI_OK;
}

extern "C" int mmi_lm_get_hidden_taps(mmi_lm* lm, void* buf, int64_t nbytes, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !buf) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming || !lm->htap) return mmi_fail(MMI_ERR_STATE, "hidden taps were not enabled before streaming_start");
    const int64_t want = (int64_t)2 * lm->batch * lm->cfg.dim * 2;
    if (nbytes != want) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_get_hidden_taps: the buffer holds " + std::to_string(nbytes) + " bytes, the taps " + std::to_string(want));
    MMI_HIP_CHECK(hipMemcpyAsync(buf, lm->htap, (size_t)want, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MMI_OK;
}

extern "C" int32_t mmi_lm_has_hooks(const mmi_lm* lm) {
    return lm && (lm->hooks.on_text_logits || lm->hooks.on_text_token || lm->hooks.on_audio_tokens) ? 1 : 0;
}

extern "C" int mmi_lm_hook_io(mmi_lm* lm, int32_t which, int32_t write, void* buf, int64_t nbytes, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !buf) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming || !lm->in_hook) return mmi_fail(MMI_ERR_STATE, "mmi_lm_hook_io is only valid inside a step hook");
    hipStream_t s = (hipStream_t)stream;
    const mmi_lm_cfg& c = lm->cfg;
    const int G = lm->gen_batch;
    const int64_t want = which == 0 ? (int64_t)G * c.text_card_out * 2 : which == 1 ? (int64_t)G * 8 : which == 2 ? (int64_t)G * c.dep_q * 8 : -1;
    if (want >= 0 && nbytes != want)
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_hook_io: the buffer holds " + std::to_string(nbytes) + " bytes, the tensor " + std::to_string(want));
    if (which == 0) {            // (guided) text logits, rows [0, G) of the model's logits buffer
        const size_t n = (size_t)G * c.text_card_out * sizeof(uint16_t);
        if (write) MMI_HIP_CHECK(hipMemcpyAsync(lm->text_logits, buf, n, hipMemcpyDeviceToDevice, s));
        else MMI_HIP_CHECK(hipMemcpyAsync(buf, lm->text_logits, n, hipMemcpyDeviceToDevice, s));
        return MMI_OK;
    }
    int* tok = which == 1 ? lm->text_tok : (which == 2 ? lm->audio_tok : nullptr);
    if (!tok) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_hook_io: which must be 0, 1 or 2");
    const int cols = which == 1 ? 1 : c.dep_q;
    if (cols == 0) return MMI_OK;
    if (write) MMI_LAUNCH(k_i64_to_i32, mmi_cdiv(G * cols, 256), 256, 0, s, (const long*)buf, (long)cols, tok, G, cols);
    else MMI_LAUNCH(k_i32_to_i64, mmi_cdiv(G * cols, 256), 256, 0, s, (const int*)tok, (long*)buf, G * cols);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

extern "C" int mmi_lm_force_next_tokens(mmi_lm* lm, const int64_t* tokens, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !tokens) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    hipStream_t s = (hipStream_t)stream;
    const int n = lm->gen_batch * (1 + lm->cfg.dep_q);
    MMI_LAUNCH(k_i64_to_i32, mmi_cdiv(n, 256), 256, 0, s, (const long*)tokens, (long)(1 + lm->cfg.dep_q), lm->forced, lm->gen_batch, 1 + lm->cfg.dep_q);
    MMI_CHECK_LAUNCH();
    MMI_HIP_CHECK(hipMemsetAsync(lm->use_forced, 1, 1, s));
    lm->forced_armed = true;
    return MMI_OK;
}

extern "C" int64_t mmi_lm_state_bytes(const mmi_lm* lm) { return lm && lm->streaming ? (int64_t)lm->st.bytes : 0; }

extern "C" int mmi_lm_state_save(mmi_lm* lm, void* dst, int64_t bytes, int64_t* host_word, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !dst || !host_word) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if (bytes != (int64_t)lm->st.bytes) return mmi_fail(MMI_ERR_SHAPE, "snapshot buffer has the wrong size");
    MMI_HIP_CHECK(lm->st.save(dst, (hipStream_t)stream));
    *host_word = lm->offset_cpu;
    return MMI_OK;
}

extern "C" int mmi_lm_state_load(mmi_lm* lm, const void* src, int64_t bytes, int64_t host_word, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !src) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    if (bytes != (int64_t)lm->st.bytes) return mmi_fail(MMI_ERR_SHAPE, "snapshot taken from a different stream (batch / guidance)");
    MMI_HIP_CHECK(lm->st.load(src, (hipStream_t)stream));
    lm->offset_cpu = (long)host_word;
    {   // the snapshot's offsets bound the ring depth (which step program the next steps take): read them back - a restore is not
        // a per-frame call, and without this a shallow restored session paid the merge launch for the rest of the stream
        std::vector<long> off(lm->batch);
        MMI_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        MMI_HIP_CHECK(hipMemcpy(off.data(), lm->offsets_m, (size_t)lm->batch * sizeof(long), hipMemcpyDeviceToHost));
        long mx = 0;
        for (long o : off) mx = o > mx ? o : mx;
        lm->depth_bound = mx;
        std::vector<RowSamp> tab(lm->gen_batch);         // and the restored table says which rows have settings of their own
        MMI_HIP_CHECK(hipMemcpy(tab.data(), lm->rowtab, tab.size() * sizeof(RowSamp), hipMemcpyDeviceToHost));
        for (int b = 0; b < lm->gen_batch; ++b) lm->row_active[b] = tab[b].active ? 1 : 0;
        if (lm->nucleus_live)                             // and the sessions' top_p (supplied noise is refused by the mirror)
            MMI_HIP_CHECK(hipMemcpy(lm->row_top_p.data(), lm->rowtab + lm->gen_batch, lm->row_top_p.size() * sizeof(RowTopP), hipMemcpyDeviceToHost));
        if (lm->row_slot)                                 // and which adapter slots are in use
            MMI_HIP_CHECK(hipMemcpy(lm->row_slot_h.data(), lm->row_slot, (size_t)lm->gen_batch * sizeof(int), hipMemcpyDeviceToHost));
    }
    lm->forced_armed = false;
    lm->noise_on = true;               // the snapshot carries its own use_noise word: the next step rewrites it
    return clear_logprobs(lm, (hipStream_t)stream, nullptr);      // a snapshot carries no log-probabilities
}

extern "C" int mmi_lm_extra_heads(mmi_lm* lm, float* probs, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !probs) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    const mmi_lm_cfg& c = lm->cfg;
    if (c.extra_heads_num_heads <= 0) return MMI_OK;
    MMI_LAUNCH(k_extra_heads, dim3(lm->batch, c.extra_heads_num_heads), 64, 0, (hipStream_t)stream, (const uint16_t*)lm->tout, lm->T,
               packed_ksteps(lm, c.dim), (const uint16_t*)lm->extra_heads_all, c.dim, c.extra_heads_dim, c.extra_heads_num_heads, probs);
    MMI_CHECK_LAUNCH();
    return MMI_OK;
}

extern "C" int mmi_lm_model_rows(const mmi_lm* lm) { return lm ? lm->batch : 0; }
extern "C" int mmi_lm_streaming_batch(const mmi_lm* lm) { return lm && lm->streaming ? lm->gen_batch : 0; }
extern "C" int mmi_lm_device(const mmi_lm* lm) { return lm ? lm->device : -1; }

int64_t mmi_copy_launch_log(const std::vector<std::string>& log, char* buf, int64_t cap);   // api_common.hip

extern "C" int64_t mmi_lm_launch_list(const mmi_lm* lm, char* buf, int64_t cap) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !lm->streaming || !lm->prog.logged()) return 0;
    return mmi_copy_launch_log(lm->prog.launch_log(), buf, cap);
}

extern "C" int mmi_lm_seek(mmi_lm* lm, const int64_t* offsets, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !offsets) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return mmi_fail(MMI_ERR_STATE, "not streaming");
    const int G = lm->gen_batch;
    std::vector<long> off(lm->batch);
    long mx = 0;
    for (int b = 0; b < G; ++b) {
        if (offsets[b] < 0) return mmi_fail(MMI_ERR_INVALID, "negative offset");
        off[b] = (long)offsets[b];
        if (lm->batch > G) off[G + b] = off[b];      // the guidance twins follow their session
        mx = off[b] > mx ? off[b] : mx;
    }
    hipStream_t s = (hipStream_t)stream;
    MMI_HIP_CHECK(hipStreamSynchronize(s));
    MMI_HIP_CHECK(hipMemcpy(lm->offsets, off.data(), (size_t)G * sizeof(long), hipMemcpyHostToDevice));
    if (lm->offsets_m != lm->offsets) MMI_HIP_CHECK(hipMemcpy(lm->offsets_m, off.data(), (size_t)lm->batch * sizeof(long), hipMemcpyHostToDevice));
    lm->offset_cpu = mx;
    lm->depth_bound = mx;
    return clear_logprobs(lm, s, nullptr);
}

// Test aids of the KV ring (include/moshi_mi.h)
extern "C" int mmi_lm_debug_kv4_quantize(mmi_lm* lm, const void* x_bf16, int32_t n, int32_t m, void* codes_u8, void* scales_u8, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !x_bf16 || !codes_u8 || !scales_u8) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (n <= 0 || m <= 0) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_kv4_quantize: n and m must be positive");
    hipStream_t s = (hipStream_t)stream;
    const long nblocks = (long)n * m;
    MMI_LAUNCH(k_kv4_quantize, (int)mmi_cdiv(nblocks, 256L), 256, 0, s, (const uint16_t*)x_bf16, nblocks, (uint8_t*)codes_u8, (uint8_t*)scales_u8);
    MMI_CHECK_LAUNCH();
    MMI_HIP_CHECK(hipStreamSynchronize(s));
    return MMI_OK;
}

extern "C" int64_t mmi_lm_debug_kv_ring(mmi_lm* lm, int32_t layer, int32_t which, void* dst, int64_t nbytes, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return (int64_t)mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!lm->streaming) return (int64_t)mmi_fail(MMI_ERR_STATE, "not streaming");
    const mmi_lm_cfg& c = lm->cfg;
    if (layer < 0 || layer >= c.num_layers || (which != 0 && which != 1))
        return (int64_t)mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_kv_ring: layer must be a temporal layer, which 0 (keys) or 1 (values)");
    const KvRing& r = lm->ring;
    const int64_t want = (int64_t)(r.codes_bytes + (r.form == 2 ? r.elems / 16 : 0));   // without the layer's padding
    if (!dst) return want;
    if (nbytes != want)
        return (int64_t)mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_kv_ring: the buffer holds " + std::to_string(nbytes) + " bytes, the layer's ring " + std::to_string(want));
    hipStream_t s = (hipStream_t)stream;
    const uint16_t* src = (which == 0 ? lm->kc : lm->vc) + (size_t)layer * r.layer_u16;
    hipError_t e = hipMemcpyAsync(dst, src, (size_t)want, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return (int64_t)mmi_fail(MMI_ERR_HIP, std::string("mmi_lm_debug_kv_ring: ") + hipGetErrorString(e));
    return want;
}

// Parity tap: ONE linear of the model on caller-supplied rows, through the kernels the step uses for it (include/moshi_mi.h).
// Works on its own scratch (TapScratch) and synchronises.
// row_slots (mmi_lm_debug_linear_lora): the rows' adapter slots, a host array - the shrink launch, then the linear with its tail
static int debug_linear_impl(mmi_lm* lm, const char* weight_name, const char* alpha_name, int32_t path, const void* x_bf16,
                             int32_t rows, void* out_bf16, int8_t* codes, float* absmax, void* norm_out, const int32_t* row_slots,
                             mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !weight_name || !x_bf16 || !out_bf16) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (row_slots) {
        if (!lm->lora_on) return mmi_fail(MMI_ERR_STATE, "mmi_lm_debug_linear_lora: the handle has no adapters (mmi_lm_enable_adapters)");
        if (path != MMI_DBG_PLAIN && path != MMI_DBG_SPLITK)
            return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_linear_lora: an adapter handle runs the plain and the split-K path");
        for (int b = 0; b < rows; ++b)
            if (row_slots[b] < -1 || row_slots[b] >= lm->lora_S) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_linear_lora: slot must be -1 (none) or in [0, max_adapters)");
    }
    if (rows <= 0 || rows > lm->max_batch) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_linear: rows must be 1..max_batch");
    auto it = lm->linear_by_name.find(weight_name);
    if (it == lm->linear_by_name.end()) return mmi_fail(MMI_ERR_MISSING_WEIGHT, std::string("no packed linear named ") + weight_name);
    const GemmW g = it->second;
    const uint16_t* alpha = nullptr;
    const bool normed = path == MMI_DBG_NORM || path == MMI_DBG_NORM_FUSED;
    if (normed) {
        auto ia = alpha_name ? lm->vector_by_name.find(alpha_name) : lm->vector_by_name.end();
        if (ia == lm->vector_by_name.end()) return mmi_fail(MMI_ERR_MISSING_WEIGHT, "mmi_lm_debug_linear: the norm's alpha vector was not found");
        alpha = ia->second;
    }
    const bool a8 = act8_of(lm);
    if ((codes || absmax) && !(a8 && (path == MMI_DBG_PLAIN || path == MMI_DBG_SPLITK || path == MMI_DBG_NORM)))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_linear: codes / absmax exist on the int8 x int8 paths that materialise the operand (plain, split-K, norm)");
    hipStream_t s = (hipStream_t)stream;
    const int T = g.T, mt = mmi_cdiv(rows, T);
    if (mt > 2 && (path == MMI_DBG_FUSED || path == MMI_DBG_NORM_FUSED))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_linear: the fused forms are not selected above 64 rows (k_gemm_rows + a norm launch)");
    const int K = g.K, N = g.N, kin = packed_ksteps_t(lm, T, K), kout = packed_ksteps_t(lm, T, N);
    TapScratch scratch(lm, s, row_slots ? "mmi_lm_debug_linear_lora" : "mmi_lm_debug_linear");
    uint16_t *xp = nullptr, *yp = nullptr, *xres = nullptr, *zeros = nullptr, *outp = (uint16_t*)out_bf16;
    uint8_t* xq = nullptr;
    float *sx = nullptr, *partial = nullptr;
    int rc;
    if ((rc = scratch.packed(&xp, rows, T, kin)) || (rc = scratch.packed(&yp, rows, T, kin)) ||
        (rc = scratch.zeroed(&xq, (size_t)mt * (kin / 2 + 1) * 1024)) || (rc = scratch.zeroed(&sx, (size_t)mt * T)) ||
        (rc = scratch.packed(&xres, rows, T, kout)) || (rc = scratch.zeroed(&zeros, (size_t)N + 8)) ||
        (rc = scratch.alloc(&partial, (size_t)4 * rows * N)))
        return rc;
    MMI_LAUNCH(k_pack_rows, mmi_cdiv(rows * K, 256), 256, 0, s, (const uint16_t*)x_bf16, rows, K, xp, T, kin);
    MMI_CHECK_LAUNCH();
    int* slots_dev = nullptr;
    uint16_t* lora_t = nullptr;
    if (row_slots) {
        if ((rc = scratch.alloc(&slots_dev, (size_t)rows)) || (rc = scratch.packed(&lora_t, rows, T, lm->lora_S * lm->lora_R / mmi_kstep(T)))) return rc;
        MMI_HIP_CHECK(hipMemcpyAsync(slots_dev, row_slots, (size_t)rows * sizeof(int), hipMemcpyHostToDevice, s));
    }
    const uint16_t* operand = xp;              // the packed bf16 rows the GEMM (or its quantiser) reads
    const bool gated = g.gate != 0;
    GemmArgs a = gemm_args(lm, T, nullptr, gated ? MMI_EPI_GATE : MMI_EPI_STORE, rows, rows, {outp, N});
    if (path == MMI_DBG_NORM) {                // the norm launch of the step: y (+ its int8 copy) = rms_norm(x) * alpha
        if ((rc = launch_rmsnorm(s, rows, xp, nullptr, Pending{}, alpha, yp, K, T, kin, a8 ? xq : nullptr, a8 ? sx : nullptr))) return rc;
        operand = yp;
        if (norm_out) MMI_LAUNCH(k_unpack_rows, mmi_cdiv(rows * K, 256), 256, 0, s, (const uint16_t*)yp, rows, K, (uint16_t*)norm_out, T, kin);
    } else if (a8 && (path == MMI_DBG_PLAIN || path == MMI_DBG_SPLITK)) {
        MMI_LAUNCH(k_quant_rows_i8, rows, row_threads(K), 0, s, (const uint16_t*)xp, rows, K, T, kin, xq, sx);
        MMI_CHECK_LAUNCH();
    }
    if (path == MMI_DBG_PLAIN || path == MMI_DBG_NORM || path == MMI_DBG_SPLITK) {
        a.xp = reinterpret_cast<const u32x4*>(operand);
        if (a8) { a.xp = reinterpret_cast<const u32x4*>(xq); a.sx = sx; a.wq = 3; }
        Pending pd;
        if (path == MMI_DBG_SPLITK) {
            const GemmPlan p = plan_gemm(lm->knobs, g, true);
            if (gated || p.ksplit <= 1) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_linear: the engine does not split this GEMM over K");
            a.epi = MMI_EPI_PARTIAL; a.partial = partial; a.out = nullptr;
            pd.P = p.ksplit;
            if (a8) { pd.sx = sx; pd.scb = g.scb; }
        }
        if (row_slots && (rc = launch_lora_shrink(lm, s, g, a.xp, rows, slots_dev, rows, lora_t))) return rc;
        if ((rc = launch_gemm(lm, s, g, a, false, reinterpret_cast<const u32x4*>(lora_t)))) return rc;
        if (path == MMI_DBG_SPLITK) {          // the fold of the next norm launch: x (= 0) + bf16(sum of the partials)
            if (N > 8 * 1024 * MMI_NORM_MAXP) return mmi_fail(MMI_ERR_UNSUPPORTED, "row too long for the norm kernel");
            uint16_t* ytmp = nullptr;
            if ((rc = scratch.alloc(&ytmp, (size_t)mt * kout * 512))) return rc;
            if ((rc = launch_rmsnorm(s, rows, xres, partial, pd, zeros, ytmp, N, T, kout))) return rc;
            MMI_LAUNCH(k_unpack_rows, mmi_cdiv(rows * N, 256), 256, 0, s, (const uint16_t*)xres, rows, N, outp, T, kout);
            MMI_CHECK_LAUNCH();
        }
    } else if (path == MMI_DBG_FUSED) {
        const int kmax = q8_fused_kmax(g);
        if (!a8 || !kmax) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_linear: k_gemm_q8 needs an int8 x int8 model and rows of <= 88 entries");
        a.xp = reinterpret_cast<const u32x4*>(xp);
        bind_weight(a, g);
        a.wq = 3;
        a.osplit = q8_fused_osplit(lm->knobs, g, a.epi, T);
        if ((rc = launch_q8_fused(s, T, mt, kmax, g.NT * a.osplit, !lm->knobs.q8_tiles_serial, a))) return rc;
    } else if (path == MMI_DBG_NORM_FUSED) {
        const int wq = (a8 && g.wq == 1) ? 3 : g.wq;
        if (g.KSTEPS > norm_fused_max(wq)) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_linear: the row is too long for the norm-fused GEMM");
        a.xp = reinterpret_cast<const u32x4*>(xp);
        a.alpha = alpha; a.D = K; a.eps = 1e-8f;
        bind_weight(a, g);
        a.wq = wq; a.osplit = 1;
        if ((rc = launch_norm_fused(s, T, mt, wq, g.NT, !lm->knobs.q8_tiles_serial, a))) return rc;
    } else {
        return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_linear: unknown path");
    }
    if (codes) MMI_LAUNCH(k_unpack_q8, mmi_cdiv(rows * K, 256), 256, 0, s, (const uint8_t*)xq, rows, K, codes, T, kin);
    if (absmax) MMI_HIP_CHECK(hipMemcpyAsync(absmax, sx, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    MMI_CHECK_LAUNCH();
    if (hipStreamSynchronize(s) != hipSuccess) return mmi_fail(MMI_ERR_HIP, "mmi_lm_debug_linear: the launches failed");
    return MMI_OK;
}

extern "C" int mmi_lm_debug_linear(mmi_lm* lm, const char* weight_name, const char* alpha_name, int32_t path, const void* x_bf16,
                                   int32_t rows, void* out_bf16, int8_t* codes, float* absmax, void* norm_out, mmi_stream stream) {
    return debug_linear_impl(lm, weight_name, alpha_name, path, x_bf16, rows, out_bf16, codes, absmax, norm_out, nullptr, stream);
}

extern "C" int mmi_lm_debug_linear_lora(mmi_lm* lm, const char* weight_name, const char* alpha_name, int32_t path, const void* x_bf16,
                                        int32_t rows, void* out_bf16, int8_t* codes, float* absmax, void* norm_out, const int32_t* row_slots,
                                        mmi_stream stream) {
    if (!row_slots) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_linear_lora: null row_slots");
    return debug_linear_impl(lm, weight_name, alpha_name, path, x_bf16, rows, out_bf16, codes, absmax, norm_out, row_slots, stream);
}

// Parity tap of the temporal decode attention (include/moshi_mi.h): launch_attn - the L.attn op - on caller-supplied operands, with
// scratch of its own for the partials, the arrival counters and the packed output.  Nothing of the handle but its device, its row
// limit and its poison knob is read.
extern "C" int mmi_lm_debug_attn(mmi_lm* lm, const void* q_bf16, const void* k_ring, const void* v_ring, const int64_t* offsets, int32_t rows,
                                 int32_t H, int32_t Dh, int32_t cap, int32_t context, int32_t kv_dtype, int32_t kernel, int32_t NS, int32_t merge,
                                 int32_t solo_rows, void* out_bf16, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !q_bf16 || !k_ring || !v_ring || !offsets || !out_bf16) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (kv_dtype != MMI_BF16 && kv_dtype != MMI_F8E4M3 && kv_dtype != MMI_F4E2M1X2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_attn: the ring is bf16, e4m3 or 4-bit (MMI_F4E2M1X2)");
    const int kvf = kv_form(kv_dtype);
    if (kvf == 2 && Dh % 32 != 0) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_attn: a 4-bit ring needs a head dim that is a multiple of 32");
    if (Dh != 32 && Dh != 64 && Dh != 128) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_attn: head dim must be 32, 64 or 128");
    if (rows <= 0 || rows > lm->max_batch) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_attn: rows must be 1..max_batch");
    if (H <= 0 || H > 1024 || cap <= 0 || cap > (1 << 20) || context <= 0 || context > cap)
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_attn: 1 <= H <= 1024, 1 <= context <= cap <= 2^20");
    if (NS < 1 || NS > 16) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_attn: 1 <= NS <= 16");
    if ((kernel != MMI_ATTN_WAVE && kernel != MMI_ATTN_SPLIT) || (merge != MMI_ATTN_MERGE_LAUNCH && merge != MMI_ATTN_MERGE_KERNEL))
        return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_attn: unknown kernel or merge");
    const bool wave = kernel == MMI_ATTN_WAVE;
    if (!wave && NS > 1 && merge == MMI_ATTN_MERGE_KERNEL)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_attn: only k_lm_attn_wave merges its partials itself");
    // 16-byte loads of the query and of ring rows (a row is a multiple of 16 bytes; so is a 4-bit codes plane, which puts the 2-byte
    // scale loads on even addresses); 8-byte offsets; bf16 stores
    if (((uintptr_t)q_bf16 | (uintptr_t)k_ring | (uintptr_t)v_ring) % 16 || (uintptr_t)offsets % 8 || (uintptr_t)out_bf16 % 2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_attn: q, k and v must be 16-byte aligned, offsets 8-byte, out 2-byte");
    hipStream_t s = (hipStream_t)stream;
    // an offset below 0 would put the clamped loads in front of the ring
    std::vector<int64_t> off((size_t)rows);
    MMI_HIP_CHECK(hipStreamSynchronize(s));
    MMI_HIP_CHECK(hipMemcpy(off.data(), offsets, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < rows; ++b)
        if (off[b] < 0) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_attn: negative offset");
    const int d = H * Dh, T = rows <= 16 ? 16 : 32, ksteps = mmi_cdiv(d, mmi_kstep(T));
    const size_t pairs = (size_t)rows * H;
    TapScratch scratch(lm, s, "mmi_lm_debug_attn");
    float *opart = nullptr, *ml = nullptr;
    unsigned* arrived = nullptr;
    uint16_t* att = nullptr;
    int rc;
    if ((rc = scratch.alloc(&opart, pairs * NS * Dh)) || (rc = scratch.alloc(&ml, pairs * NS * 2)) || (rc = scratch.zeroed(&arrived, pairs)) ||
        (rc = scratch.packed(&att, rows, T, ksteps)))
        return rc;
    LmAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.qrot = (uint16_t*)q_bf16; a.kc = (uint16_t*)k_ring; a.vc = (uint16_t*)v_ring;
    a.offsets = reinterpret_cast<const long*>(offsets); a.opart = opart; a.ml = ml; a.out = att;
    a.B = rows; a.H = H; a.Dh = Dh; a.cap = cap; a.context = context; a.NS = NS;
    a.T = T; a.out_ksteps = ksteps;
    a.done = arrived; a.solo_rows = solo_rows;
    a.kv_soff = kvf == 2 ? (long)pairs * cap * Dh / 2 : 0;
    if ((rc = launch_attn(s, a, kvf, wave, NS > 1 && merge == MMI_ATTN_MERGE_LAUNCH))) return rc;
    return scratch.unpack(att, rows, d, T, ksteps, out_bf16);
}

// Parity tap of the depth transformer's attention (include/moshi_mi.h): launch_dep_attn - the step's dep.attn op and the scoring
// pass's - on caller-supplied operands, with a packed output of its own.  Nothing of the handle but its device, its row limit and its
// poison knob is read.
static int debug_rows_bound(const mmi_lm* lm) { return lm->max_batch > 128 ? lm->max_batch : 128; }

extern "C" int mmi_lm_debug_dep_attn(mmi_lm* lm, const void* qkv_bf16, void* k_cache, void* v_cache, int32_t rows, int32_t H, int32_t Dh,
                                     int32_t steps, int32_t k, int32_t kernel, void* out_bf16, int32_t* kernel_run, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !qkv_bf16 || !k_cache || !v_cache || !out_bf16) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_dep_attn: null argument");
    if (kernel != MMI_DEP_ATTN_AUTO && kernel != MMI_DEP_ATTN_8 && kernel != MMI_DEP_ATTN_ROWS16 && kernel != MMI_DEP_ATTN_ROWS32)
        return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_dep_attn: unknown kernel");
    if (Dh < 1 || Dh > 64) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_dep_attn: head dim must be 1..64");
    if (steps < 1 || steps > 32) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_dep_attn: steps must be 1..32");
    if (k < 0 || k >= steps) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_dep_attn: k must be in [0, steps)");
    if (H < 1 || H > 1024) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_dep_attn: 1 <= H <= 1024");
    if (rows < 1 || rows > debug_rows_bound(lm))
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_dep_attn: rows must be 1.." + std::to_string(debug_rows_bound(lm)) + " (128, or the handle's max_batch above it)");
    if (kernel == MMI_DEP_ATTN_8 && (Dh % 8 || steps > 8))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_dep_attn: k_dep_attn8 needs a head dim that is a multiple of 8 and steps <= 8");
    if (kernel == MMI_DEP_ATTN_ROWS16 && steps > 16)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_dep_attn: k_dep_attn<16> holds 16 cache rows: steps <= 16");
    // 16-byte loads and stores of qkv and cache pieces (k_dep_attn8); bf16 stores of the result
    if (((uintptr_t)qkv_bf16 | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 || (uintptr_t)out_bf16 % 2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_dep_attn: qkv and the caches must be 16-byte aligned, out 2-byte");
    hipStream_t s = (hipStream_t)stream;
    const int d = H * Dh, T = rows <= 16 ? 16 : 32, ksteps = mmi_cdiv(d, mmi_kstep(T));
    TapScratch scratch(lm, s, "mmi_lm_debug_dep_attn");
    uint16_t* att = nullptr;
    int rc = scratch.packed(&att, rows, T, ksteps);
    if (rc) return rc;
    DepAttnArgs da;
    da.qkv = (const uint16_t*)qkv_bf16; da.kc = (uint16_t*)k_cache; da.vc = (uint16_t*)v_cache; da.out = att;
    da.B = rows; da.H = H; da.Dh = Dh; da.steps = steps; da.k = k; da.T = T; da.out_ksteps = ksteps;
    int ran = -1;
    if ((rc = launch_dep_attn(s, da, kernel, &ran)) || (rc = scratch.unpack(att, rows, d, T, ksteps, out_bf16))) return rc;
    if (kernel_run) *kernel_run = ran;
    return MMI_OK;
}

// The same for the attention inside out_proj: depth layer `layer`, micro-step k >= 1 of the handle's own model, ONE row.  fused != 0:
// the launch and plan of add_dep_attn_out_proj; else the two launches it replaces - launch_dep_attn, then out_proj through
// launch_gemm with the arguments add_gemm gives it.
extern "C" int mmi_lm_debug_dep_attn_out_proj(mmi_lm* lm, int32_t layer, int32_t k, int32_t fused, const void* qkv_bf16, void* k_cache,
                                              void* v_cache, const void* x_bf16, void* out_bf16, void* att_bf16, int32_t* kernel_run,
                                              mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !qkv_bf16 || !k_cache || !v_cache || !x_bf16 || !out_bf16) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_dep_attn_out_proj: null argument");
    const mmi_lm_cfg& c = lm->cfg;
    if (layer < 0 || layer >= c.depformer_num_layers) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_dep_attn_out_proj: layer must be in [0, depformer_num_layers)");
    if (k < 1 || k >= c.dep_q) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_dep_attn_out_proj: k must be in [1, dep_q) (micro-step 0 has no attention launch)");
    const int dd = c.depformer_dim, H = c.depformer_num_heads, Dh = dd / H, steps = c.dep_q;
    const GemmW g = lm->dep_layers[layer].out_proj[k];
    if (!dep_attn_fusable(lm, g, H, Dh, steps, 1))
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_dep_attn_out_proj: the engine does not run this out_proj with the attention inside (dep_attn_fusable)");
    if (((uintptr_t)qkv_bf16 | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 || ((uintptr_t)x_bf16 | (uintptr_t)out_bf16 | (uintptr_t)att_bf16) % 2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_dep_attn_out_proj: qkv and the caches must be 16-byte aligned, x and out 2-byte");
    hipStream_t s = (hipStream_t)stream;
    const int T = g.T, ksteps = packed_ksteps_t(lm, T, dd);
    TapScratch scratch(lm, s, "mmi_lm_debug_dep_attn_out_proj");
    uint16_t *xp = nullptr, *att = nullptr;
    int ran = -1, rc;
    if ((rc = scratch.packed(&xp, 1, T, ksteps)) || (rc = scratch.packed(&att, 1, T, ksteps))) return rc;
    MMI_LAUNCH(k_pack_rows, mmi_cdiv(dd, 256), 256, 0, s, (const uint16_t*)x_bf16, 1, dd, xp, T, ksteps);
    MMI_CHECK_LAUNCH();
    DepAttnArgs da;
    da.qkv = (const uint16_t*)qkv_bf16; da.kc = (uint16_t*)k_cache; da.vc = (uint16_t*)v_cache; da.out = att;
    da.B = 1; da.H = H; da.Dh = Dh; da.steps = steps; da.k = k; da.T = T; da.out_ksteps = ksteps;
    if (fused) {
        rc = launch_dep_attn_out_proj_planned(s, plan_dep_attn_out_proj(lm, g, xp, dd, 1, 1), da);
        ran = MMI_DEP_ATTN_FUSED;
    } else {
        if ((rc = launch_dep_attn(s, da, MMI_DEP_ATTN_AUTO, &ran))) return rc;
        // the step's add_gemm(lm, out_proj, datt, MMI_EPI_RESID, {dx, dd, true}) with resid = dx, on one row
        rc = launch_gemm(lm, s, g, gemm_args(lm, T, att, MMI_EPI_RESID, 1, 1, {xp, dd, true}, xp), false);
    }
    if (rc) return rc;
    if (att_bf16 && !fused) MMI_LAUNCH(k_unpack_rows, mmi_cdiv(dd, 256), 256, 0, s, (const uint16_t*)att, 1, dd, (uint16_t*)att_bf16, T, ksteps);
    if ((rc = scratch.unpack(xp, 1, dd, T, ksteps, out_bf16))) return rc;
    if (kernel_run) *kernel_run = ran;
    return MMI_OK;
}

// Parity tap of the cross attention (include/moshi_mi.h): launch_cross_attn - the L.cross_attn op - on caller-supplied operands.
extern "C" int mmi_lm_debug_cross_attn(mmi_lm* lm, const void* q_bf16, const void* kv_bf16, const int32_t* len, int32_t rows, int32_t H,
                                       int32_t Dh, int32_t cap, void* out_bf16, mmi_stream stream) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !q_bf16 || !kv_bf16 || !len || !out_bf16) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_cross_attn: null argument");
    if (Dh != 32 && Dh != 64 && Dh != 128) return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_cross_attn: head dim must be 32, 64 or 128");
    if (rows < 1 || rows > debug_rows_bound(lm))
        return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_cross_attn: rows must be 1.." + std::to_string(debug_rows_bound(lm)) + " (128, or the handle's max_batch above it)");
    if (H < 1 || H > 1024 || cap < 1 || cap > (1 << 20)) return mmi_fail(MMI_ERR_SHAPE, "mmi_lm_debug_cross_attn: 1 <= H <= 1024, 1 <= cap <= 2^20");
    if (((uintptr_t)q_bf16 | (uintptr_t)kv_bf16) % 16 || (uintptr_t)len % 4 || (uintptr_t)out_bf16 % 2)
        return mmi_fail(MMI_ERR_UNSUPPORTED, "mmi_lm_debug_cross_attn: q and kv must be 16-byte aligned, len 4-byte, out 2-byte");
    hipStream_t s = (hipStream_t)stream;
    // a length outside [1, cap] would put the loads (the clamped ones: row len - 1) outside the row's positions
    std::vector<int32_t> L((size_t)rows);
    MMI_HIP_CHECK(hipStreamSynchronize(s));
    MMI_HIP_CHECK(hipMemcpy(L.data(), len, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < rows; ++b)
        if (L[b] < 1 || L[b] > cap) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_debug_cross_attn: every len must be in [1, cap]");
    const int d = H * Dh, T = rows <= 16 ? 16 : 32, ksteps = mmi_cdiv(d, mmi_kstep(T));
    TapScratch scratch(lm, s, "mmi_lm_debug_cross_attn");
    uint16_t* att = nullptr;
    int rc = scratch.packed(&att, rows, T, ksteps);
    if (rc) return rc;
    CrossAttnArgs ca;
    ca.q = (const uint16_t*)q_bf16; ca.kv = (const uint16_t*)kv_bf16; ca.out = att; ca.len = len;
    ca.B = rows; ca.H = H; ca.Dh = Dh; ca.cap = cap; ca.T = T; ca.out_ksteps = ksteps;
    if ((rc = launch_cross_attn(s, ca))) return rc;
    return scratch.unpack(att, rows, d, T, ksteps, out_bf16);
}

extern "C" int64_t mmi_lm_stat(const mmi_lm* lm, int32_t which) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return -1;
    if (which == 0) return (int64_t)lm->xlds_launches;
    if (which == 1) {       // bit v set: step program v (attn_variant) is captured and instantiated (either graph form)
        int64_t m = 0;
        for (int v = 0; v < MmiProgram::NV; ++v)
            if (lm->prog.ready(v, false) || lm->prog.ready(v, true)) m |= 1ll << v;
        return m;
    }
    if (which == 2) return (int64_t)lm->depth_bound;
    if (which == 3) return (int64_t)lm->Td;               // the depth transformer's MFMA tile (16 / 32)
    if (which == 4) return (int64_t)lm->rows_launches;
    return -1;
}

extern "C" int mmi_lm_profile_begin(mmi_lm* lm) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    lm->profiling = true;
    lm->ev_used = 0;
    lm->site_ev_used = 0;
    lm->prog.tap = [lm](size_t i, bool begin, hipStream_t s) {       // one event per op boundary of the un-graphed steps
        if (!begin && i + 1 != lm->prog.ops.size()) return;
        if (lm->site_ev_used == lm->site_ev.size()) {
            mmi_lm::SiteEv e{0, nullptr};
            if (hipEventCreate(&e.ev) != hipSuccess) return;
            lm->site_ev.push_back(e);
        }
        lm->site_ev[lm->site_ev_used].op = begin ? i : (size_t)-1;
        hipEventRecord(lm->site_ev[lm->site_ev_used].ev, s);
        lm->site_ev_used += 1;
    };
    return MMI_OK;
}

// Per-site timings of the steps run since mmi_lm_profile_begin: one line "site<TAB>ops<TAB>total ms<TAB>weight bytes per op" per
// site of the launch list (one hipEvent per op boundary of the un-graphed steps: an op's time runs to the next op's event, so the
// eager dispatch gap and the event's own marker - a few us - are included).  Call before
// mmi_lm_profile_end; synchronises the stream.  Returns the bytes needed including the final NUL.
extern "C" int64_t mmi_lm_profile_sites(mmi_lm* lm, char* buf, int64_t cap) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm || !lm->profiling) return 0;
    if (lm->prof_stream) hipStreamSynchronize(lm->prof_stream);
    else hipDeviceSynchronize();
    std::vector<std::string> order;
    std::vector<double> tot;
    std::vector<long> cnt, bytes;
    for (size_t k = 0; k + 1 < lm->site_ev_used; ++k) {
        const auto& e = lm->site_ev[k];
        if (e.op == (size_t)-1) continue;            // the end of a step: the distance to the next step's first event is host time
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.ev, lm->site_ev[k + 1].ev) != hipSuccess) continue;
        const std::string& site = lm->prog.sites[e.op];
        size_t j = 0;
        while (j < order.size() && order[j] != site) ++j;
        if (j == order.size()) { order.push_back(site); tot.push_back(0.0); cnt.push_back(0); bytes.push_back(0); }
        tot[j] += ms; cnt[j] += 1;
        if (lm->prog.op_bytes[e.op] > bytes[j]) bytes[j] = lm->prog.op_bytes[e.op];
    }
    (void)hipGetLastError();
    std::string all;
    for (size_t j = 0; j < order.size(); ++j)
        all += order[j] + "\t" + std::to_string(cnt[j]) + "\t" + std::to_string(tot[j]) + "\t" + std::to_string(bytes[j]) + "\n";
    const int64_t need = (int64_t)all.size() + 1;
    if (buf && cap > 0) {
        const int64_t n = need <= cap ? need - 1 : cap - 1;
        memcpy(buf, all.data(), (size_t)n);
        buf[n] = 0;
    }
    return need;
}

extern "C" int mmi_lm_profile_end(mmi_lm* lm, double* mean_ms, int64_t* n_launches, int64_t* bytes_per_launch,
                                  const char** kernel_name) {
    MmiDeviceGuard dev_guard_(lm ? lm->device : -1);
    if (!lm) return mmi_fail(MMI_ERR_INVALID, "null handle");
    if (!lm->profiling) return mmi_fail(MMI_ERR_STATE, "profiling was not started");
    lm->profiling = false;
    lm->prog.tap = nullptr;
    if (lm->prof_stream || lm->ev_used) MMI_HIP_CHECK(hipStreamSynchronize(lm->prof_stream));
    double tot = 0.0;
    for (size_t i = 0; i < lm->ev_used; ++i) {
        float ms = 0.f;
        MMI_HIP_CHECK(hipEventElapsedTime(&ms, lm->ev_pool[i].a, lm->ev_pool[i].b));
        tot += ms;
    }
    if (mean_ms) *mean_ms = lm->ev_used ? tot / (double)lm->ev_used : 0.0;
    if (n_launches) *n_launches = (int64_t)lm->ev_used;
    if (bytes_per_launch) {
        const mmi_lm_cfg& c = lm->cfg;
        // algorithmic bytes of one FFN linear_in launch: packed weights + activations in + gated activations out
        const int64_t wbytes = lm->q8 == 4 ? (int64_t)2 * c.ffn_hidden * c.dim / 2 + (int64_t)2 * c.ffn_hidden * c.dim / 16
                               : lm->q8 >= 1 ? (int64_t)2 * c.ffn_hidden * c.dim + (int64_t)2 * c.ffn_hidden * 4 : (int64_t)2 * c.ffn_hidden * c.dim * 2;
        *bytes_per_launch = wbytes + (int64_t)lm->batch * c.dim * 2 + (int64_t)lm->batch * c.ffn_hidden * 2;
    }
    if (kernel_name)
        *kernel_name = lm->act8      ? "k_gemm_xp<32, MT, 1, 8, 2, 3> (temporal FFN linear_in, int8 weights x int8 activations on v_mfma_i32_32x32x32_i8 + SiLU gate)"
                       : lm->q8 == 1 ? "k_gemm_xp<32, 1, 1, 8, 2, 1> (temporal FFN linear_in, int8 weights + SiLU gate)"
                       : lm->q8 == 4 ? "k_gemm_xp<32, MT, 1, 8, U, 4> (temporal FFN linear_in, MXFP4 weights widened to bf16 + SiLU gate)"
                       : lm->q8 == 2 ? "k_gemm_xp<32, 1, 1, 8, 2, 2> (temporal FFN linear_in, fp8 weights on the fp8 MFMA + SiLU gate)"
                       : lm->dominant_xlds ? (lm->batch > 32 ? "k_gemm_xlds<2, 32, 3, true, 0> (temporal FFN linear_in + SiLU gate)"
                                                             : "k_gemm_xlds<1, 64, 3, true, 0> (temporal FFN linear_in + SiLU gate)")
                                     : "k_gemm_xp<32, 1, 1, 8, 2> (temporal FFN linear_in + SiLU gate)";
    lm->ev_used = 0;
    return MMI_OK;
}
