// Session batcher behind the C ABI (include/moshi_mi.h, "Session batcher"): the model loop that packs many live
// full-duplex dialogue sessions into the batched frame step of one GPU.
//
// The reference's Python server holds ONE session under an asyncio lock (moshi/moshi/server.py:45,57,154-169); the
// reference's Rust server is the model for batching: a fixed number of slots, a channel per slot with a PCM FIFO, and a
// loop that every iteration (rust/moshi-server/src/batched_asr.rs:188-276)
//   pre_process  (:279-374)  pulls one 1920-sample frame per channel that has one -> stream mask; resets newly opened rows
//   step                     runs the batched model step with that mask
//   post_process (:376-437)  routes the per-row results back to the channel that owned the row when the step started.
// Here the step is the duplex path  Mimi encode -> LMGen.step -> Mimi decode  through the public entry points only
// (this file uses nothing of the engines but include/moshi_mi.h), so it is also the worked example of driving the ABI.
#include "mmi_common.h"

#include <math.h>
#include <deque>
#include <mutex>

namespace {

struct OutFrame {
    std::vector<float> pcm;
    std::vector<int64_t> tokens;
    std::vector<float> logp, top_logp;       // mmi_lm_frame_logprobs of the frame's step (an LM handle with the option), else empty
    std::vector<int32_t> top_id;
};

struct Channel {                 // batched_asr.rs:61-69
    int64_t id = 0;
    bool live = false;
    bool pending_reset = false;  // opened since the last step: the row's streaming state is reset before it runs
    bool own_sampling = false;   // mmi_batcher_open_with: the row samples with `sampling` instead of the batcher's settings
    mmi_row_sampling sampling{};
    bool own_cond = false;       // mmi_batcher_open_cond: the row gets this condition instead of the batcher's cfg.guidance
    float coef = 1.f;
    int cross_len = 0;
    std::vector<uint16_t> cond_sum, cond_cross;   // bf16 [R][dim] / [R][cross_len][dim], copied at open; empty = keep
    int adapter = -1;            // mmi_batcher_open_lora: the row runs on this adapter slot for the channel's life
    bool own_top_p = false, top_p_dirty = false;   // mmi_batcher_set_channel_top_p: the row samples with these for the channel's life
    float top_p = 0.f, top_p_text = 0.f;
    long frames = 0;             // input frames consumed
    std::deque<float> in;        // PCM FIFO
    std::deque<OutFrame> out;
};

// One step's host<->device staging, laid out so that each direction is ONE copy.
struct Staging {
    // host -> device
    float* pcm = nullptr;        // [B][F]
    uint8_t* exec = nullptr;     // [B] rows that have a frame this step
    uint8_t* first = nullptr;    // [B] rows on their first frame (codec state dropped after the encode)
    uint8_t* reset = nullptr;    // [B] rows opened since the last step
    size_t h2d_bytes = 0;
    // device -> host
    int64_t* tokens = nullptr;   // [B][1 + dep_q]
    float* pcm_out = nullptr;    // [B][F]
    uint8_t* played = nullptr;   // [B] rows whose tokens were valid (decoder executed)
    size_t d2h_bytes = 0;
    unsigned char *up = nullptr, *down = nullptr;   // block bases
};

size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

// up / down null: only the block sizes are wanted (no pointer is formed from a null base)
void carve(Staging* st, unsigned char* up, unsigned char* down, int B, int F, int NTOK) {
    auto at = [](unsigned char* base, size_t o) -> unsigned char* { return base ? base + o : nullptr; };
    size_t o = 0;
    st->up = up;
    st->pcm = reinterpret_cast<float*>(at(up, o)); o += align_up((size_t)B * F * sizeof(float));
    st->exec = at(up, o); o += align_up(B);
    st->first = at(up, o); o += align_up(B);
    st->reset = at(up, o); o += align_up(B);
    st->h2d_bytes = o;
    o = 0;
    st->down = down;
    st->tokens = reinterpret_cast<int64_t*>(at(down, o)); o += align_up((size_t)B * NTOK * sizeof(int64_t));
    st->pcm_out = reinterpret_cast<float*>(at(down, o)); o += align_up((size_t)B * F * sizeof(float));
    st->played = at(down, o); o += align_up(B);
    st->d2h_bytes = o;
}

// out tokens [B][1 + dep_q] (-2 = not generated yet, lm.py:781-782) -> decoder exec mask and codes:
// a row's audio is decoded only when it ran this step AND its tokens are valid; the codes are clamped into the codebook
// exactly where the reference indexes them unchecked (vq.py:144-146).
__global__ void k_batcher_route(const long* __restrict__ tokens, const uint8_t* __restrict__ exec, uint8_t* __restrict__ played,
                                long* __restrict__ codes, int B, int dep_q, int card) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= B) return;
    const long* row = tokens + (long)b * (1 + dep_q);
    bool ok = exec[b] != 0;
    for (int j = 0; j <= dep_q; ++j) ok = ok && row[j] >= 0;
    for (int k = 0; k < dep_q; ++k) {
        long c = row[1 + k];
        codes[(long)b * dep_q + k] = c < 0 ? 0 : (c >= card ? card - 1 : c);
    }
    played[b] = ok ? 1 : 0;
}

}  // namespace

struct mmi_batcher {
    mmi_mimi* mimi = nullptr;
    mmi_lm* lm = nullptr;
    mmi_batcher_cfg cfg;
    int B = 0, F = 0, K = 0, dep_q = 0, card = 0, NTOK = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool models_streaming = false;
    Staging host, dev;            // pinned host blocks and their device mirrors (same carving)
    int64_t* d_codes = nullptr;   // [B][K][1] user codes from the encoder
    int64_t* d_dec_codes = nullptr;
    std::mutex mu;                // guards channels / stats (batched_asr.rs:438 Channels = Arc<Mutex<..>>)
    std::mutex step_mu;           // held by a whole step and by a fork (taken before `mu`): their launches never interleave
    std::vector<Channel> channels;
    std::vector<int64_t> row_owner;   // channel id that owned each row when the current step started
    std::vector<uint8_t> m_set, m_clear;      // rows opened since the last step: with / without settings of their own
    std::vector<mmi_row_sampling> row_set;
    // per-channel conditions (mmi_batcher_open_cond).  A slot's region of the three blocks below is [R][dim] sum rows, then
    // [R][cross_cap][dim] source positions (packed at the channel's own length); R = model rows per session.
    bool guided = false, has_sum = false, has_cross = false;
    int R = 1, dim = 0, cross_cap = 0, cross_len0 = 0;
    float coef0 = 1.f;
    size_t cond_slot = 0;             // bf16 elements per slot region
    uint16_t* h_cond = nullptr;       // pinned staging [B] regions
    uint16_t* d_cond = nullptr;       // their device mirror
    uint16_t* d_def = nullptr;        // cfg.guidance's own rows per slot, kept to give a slot back to a channel without a condition
    struct CondPlan { int what; float coef; bool sum, cross; int len; bool prev; };   // prev: the slot's last owner had one too   // what: 0 nothing, 1 the channel's own, 2 cfg.guidance's again
    std::vector<CondPlan> cond_plan;
    std::vector<uint8_t> row_has_cond;   // the slot's rows currently hold a channel's own condition
    std::vector<int> row_adapter, adapter_plan;   // the adapter slot each row holds / takes at this step (-2: stays as it is)
    std::vector<uint8_t> row_has_top_p;  // the row currently holds a channel's own top_p
    struct TopPPlan { int what; float top_p, top_p_text; };   // what: 0 nothing, 1 the channel's values, 2 the handle's again
    std::vector<TopPPlan> top_p_plan;
    // log-probabilities (mmi_lm_enable_logprobs on the LM handle): the frame read-out of every step, device and pinned host
    bool lp_on = false;
    int lp_top_n = 0;
    float *d_lp = nullptr, *h_lp = nullptr;           // [B][NTOK]
    int32_t *d_lp_id = nullptr, *h_lp_id = nullptr;   // [B][NTOK][top_n]
    float *d_lp_top = nullptr, *h_lp_top = nullptr;
    int64_t next_id = 1;
    mmi_batcher_stats stats;
};

namespace {

Channel* find_channel(mmi_batcher* b, int64_t id) {
    for (auto& c : b->channels)
        if (c.live && c.id == id) return &c;
    return nullptr;
}

void release(mmi_batcher* b) {
    if (b->models_streaming) {
        hipStreamSynchronize(b->stream);
        mmi_lm_streaming_stop(b->lm);
        mmi_mimi_streaming_stop(b->mimi);
    }
    if (b->host.up) hipHostFree(b->host.up);
    if (b->host.down) hipHostFree(b->host.down);
    if (b->dev.up) hipFree(b->dev.up);
    if (b->dev.down) hipFree(b->dev.down);
    if (b->d_codes) hipFree(b->d_codes);
    if (b->d_dec_codes) hipFree(b->d_dec_codes);
    if (b->h_cond) hipHostFree(b->h_cond);
    if (b->d_cond) hipFree(b->d_cond);
    if (b->d_def) hipFree(b->d_def);
    for (void* p : {(void*)b->d_lp, (void*)b->d_lp_id, (void*)b->d_lp_top}) if (p) hipFree(p);
    for (void* p : {(void*)b->h_lp, (void*)b->h_lp_id, (void*)b->h_lp_top}) if (p) hipHostFree(p);
    if (b->ev_begin) hipEventDestroy(b->ev_begin);
    if (b->ev_end) hipEventDestroy(b->ev_end);
    if (b->stream) hipStreamDestroy(b->stream);
    delete b;
}

int create_impl(mmi_batcher* b) {
    mmi_mimi_cfg mc;
    mmi_lm_cfg lc;
    int rc;
    if ((rc = mmi_mimi_get_cfg(b->mimi, &mc)) || (rc = mmi_lm_get_cfg(b->lm, &lc))) return rc;
    b->F = mc.frame_size * mc.channels;
    b->K = mmi_mimi_num_codebooks(b->mimi);
    b->dep_q = lc.dep_q;
    b->card = lc.card;
    b->NTOK = 1 + lc.dep_q;
    if (b->K < lc.n_q - lc.dep_q)
        return mmi_fail(MMI_ERR_SHAPE, "the codec produces fewer codebooks than the LM expects from the user stream");   // lm.py:683-686
    // the encoder produces K = max(dep_q, n_q - dep_q) codebooks (loaders.py:284-291); the decoder takes the dep_q the LM generates
    if (lc.dep_q > mc.q_n_q) return mmi_fail(MMI_ERR_SHAPE, "the LM generates more codebooks than the codec has");
    if (mc.q_bins != lc.card) return mmi_fail(MMI_ERR_SHAPE, "codec cardinality != LM card");
    const int B = b->B;
    MMI_HIP_CHECK(hipStreamCreate(&b->stream));
    MMI_HIP_CHECK(hipEventCreate(&b->ev_begin));
    MMI_HIP_CHECK(hipEventCreate(&b->ev_end));
    Staging probe;
    carve(&probe, nullptr, nullptr, B, b->F, b->NTOK);
    unsigned char *hu = nullptr, *hd = nullptr, *du = nullptr, *dd = nullptr;
    MMI_HIP_CHECK(hipHostMalloc((void**)&hu, probe.h2d_bytes, 0));
    b->host.up = hu;
    MMI_HIP_CHECK(hipHostMalloc((void**)&hd, probe.d2h_bytes, 0));
    b->host.down = hd;
    MMI_HIP_CHECK(hipMalloc((void**)&du, probe.h2d_bytes));
    b->dev.up = du;
    MMI_HIP_CHECK(hipMalloc((void**)&dd, probe.d2h_bytes));
    b->dev.down = dd;
    carve(&b->host, hu, hd, B, b->F, b->NTOK);
    carve(&b->dev, du, dd, B, b->F, b->NTOK);
    MMI_HIP_CHECK(hipMemset(dd, 0, probe.d2h_bytes));   // rows (or, for an ASR model, the whole PCM block) nobody writes read as zero
    memset(hu, 0, probe.h2d_bytes);
    memset(hd, 0, probe.d2h_bytes);
    MMI_HIP_CHECK(hipMalloc((void**)&b->d_codes, (size_t)B * b->K * sizeof(int64_t)));
    MMI_HIP_CHECK(hipMalloc((void**)&b->d_dec_codes, (size_t)B * (b->dep_q > 0 ? b->dep_q : 1) * sizeof(int64_t)));
    int32_t lp_top_n = 0;
    b->lp_on = mmi_lm_logprobs_enabled(b->lm, &lp_top_n) == 1;
    b->lp_top_n = b->lp_on ? lp_top_n : 0;
    if (b->lp_on) {
        const size_t n = (size_t)B * b->NTOK;
        MMI_HIP_CHECK(hipMalloc((void**)&b->d_lp, n * sizeof(float)));
        MMI_HIP_CHECK(hipHostMalloc((void**)&b->h_lp, n * sizeof(float), 0));
        if (b->lp_top_n) {
            MMI_HIP_CHECK(hipMalloc((void**)&b->d_lp_id, n * b->lp_top_n * sizeof(int32_t)));
            MMI_HIP_CHECK(hipHostMalloc((void**)&b->h_lp_id, n * b->lp_top_n * sizeof(int32_t), 0));
            MMI_HIP_CHECK(hipMalloc((void**)&b->d_lp_top, n * b->lp_top_n * sizeof(float)));
            MMI_HIP_CHECK(hipHostMalloc((void**)&b->h_lp_top, n * b->lp_top_n * sizeof(float), 0));
        }
    }
    // streaming_forever(batch) on both models (server.py:59-60)
    if ((rc = mmi_mimi_streaming_start(b->mimi, B, b->stream))) return rc;
    b->models_streaming = true;
    const mmi_guidance* guide = (b->cfg.guidance.cfg_coef != 0.f && b->cfg.guidance.cfg_coef != 1.f) || b->cfg.guidance.condition_sum || b->cfg.guidance.condition_cross
                                    ? &b->cfg.guidance : nullptr;
    if (guide && guide->cfg_coef == 0.f) b->cfg.guidance.cfg_coef = 1.f;    // condition only
    if ((rc = mmi_lm_streaming_start_guided(b->lm, B, &b->cfg.sampling, guide, b->stream))) return rc;
    b->channels.resize(B);
    b->row_owner.assign(B, 0);
    b->m_set.assign(B, 0);
    b->m_clear.assign(B, 0);
    b->row_set.assign(B, mmi_row_sampling{});
    // what a channel's own condition may be, and cfg.guidance's rows regrouped per slot (the caller's buffers may go away)
    b->guided = guide && guide->cfg_coef != 1.f;
    b->R = b->guided ? 2 : 1;
    b->dim = lc.dim;
    b->coef0 = guide ? guide->cfg_coef : 1.f;
    b->has_sum = guide && guide->condition_sum;
    b->has_cross = lc.cross_attention != 0;
    b->cross_len0 = b->has_cross ? guide->cross_len : 0;
    b->cross_cap = b->has_cross ? mmi_lm_cross_capacity(b->lm) : 0;
    b->cond_slot = (size_t)b->R * b->dim * (1 + (size_t)b->cross_cap);
    b->cond_plan.assign(B, mmi_batcher::CondPlan{0, 1.f, false, false, 0, false});
    b->row_has_cond.assign(B, 0);
    b->row_adapter.assign(B, -1);
    b->adapter_plan.assign(B, -2);
    b->row_has_top_p.assign(B, 0);
    b->top_p_plan.assign(B, mmi_batcher::TopPPlan{0, 0.f, 0.f});
    if (b->has_sum || b->has_cross) {
        const size_t bytes = (size_t)B * b->cond_slot * sizeof(uint16_t), D = (size_t)b->dim;
        MMI_HIP_CHECK(hipHostMalloc((void**)&b->h_cond, bytes, 0));
        MMI_HIP_CHECK(hipMalloc((void**)&b->d_cond, bytes));
        MMI_HIP_CHECK(hipMalloc((void**)&b->d_def, bytes));
        const uint16_t* gs = reinterpret_cast<const uint16_t*>(guide->condition_sum);
        const uint16_t* gx = reinterpret_cast<const uint16_t*>(guide->condition_cross);
        for (int r = 0; r < B; ++r)
            for (int t = 0; t < b->R; ++t) {     // model row t * B + r
                uint16_t* reg = b->d_def + (size_t)r * b->cond_slot;
                if (b->has_sum)
                    MMI_HIP_CHECK(hipMemcpyAsync(reg + t * D, gs + ((size_t)t * B + r) * D, D * sizeof(uint16_t), hipMemcpyDeviceToDevice, b->stream));
                if (b->has_cross)
                    MMI_HIP_CHECK(hipMemcpyAsync(reg + b->R * D + (size_t)t * b->cross_len0 * D, gx + ((size_t)t * B + r) * b->cross_len0 * D,
                                                 (size_t)b->cross_len0 * D * sizeof(uint16_t), hipMemcpyDeviceToDevice, b->stream));
            }
        MMI_HIP_CHECK(hipStreamSynchronize(b->stream));
    }
    memset(&b->stats, 0, sizeof(b->stats));
    b->stats.total_slots = B;
    return MMI_OK;
}

}  // namespace

extern "C" int mmi_batcher_create(mmi_mimi* mimi, mmi_lm* lm, const mmi_batcher_cfg* cfg, mmi_batcher** out) {
    MmiDeviceGuard dev_guard_(lm ? mmi_lm_device(lm) : -1);
    if (!mimi || !lm || !cfg || !out) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (cfg->slots <= 0) return mmi_fail(MMI_ERR_INVALID, "slots must be positive");
    mmi_batcher* b = new mmi_batcher();
    b->mimi = mimi;
    b->lm = lm;
    b->cfg = *cfg;
    if (b->cfg.max_buffered_frames <= 0) b->cfg.max_buffered_frames = 250;   // 20 s of audio per channel
    b->B = cfg->slots;
    int rc = create_impl(b);
    if (rc) {
        release(b);
        return rc;
    }
    *out = b;
    return MMI_OK;
}

extern "C" void mmi_batcher_destroy(mmi_batcher* b) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (b) release(b);
}

extern "C" int mmi_batcher_open(mmi_batcher* b, int64_t* channel_id) { return mmi_batcher_open_with(b, nullptr, channel_id); }

extern "C" int mmi_batcher_open_with(mmi_batcher* b, const mmi_row_sampling* settings, int64_t* channel_id) {
    return mmi_batcher_open_cond(b, settings, nullptr, channel_id);
}

int mmi_lm_adapter_slots(const mmi_lm* lm);      // lm_engine.hip: max_adapters of an adapter handle, else 0

extern "C" int mmi_batcher_open_cond(mmi_batcher* b, const mmi_row_sampling* settings, const mmi_batcher_condition* cond, int64_t* channel_id) {
    return mmi_batcher_open_lora(b, settings, cond, -1, channel_id);
}

extern "C" int mmi_batcher_open_lora(mmi_batcher* b, const mmi_row_sampling* settings, const mmi_batcher_condition* cond, int32_t adapter_slot,
                                     int64_t* channel_id) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b || !channel_id) return mmi_fail(MMI_ERR_INVALID, "null argument");
    int rc;
    if (adapter_slot != -1) {     // what mmi_lm_set_row_adapter would refuse at the step, refused now
        const int S = mmi_lm_adapter_slots(b->lm);
        if (!S) return mmi_fail(MMI_ERR_STATE, "adapters are not enabled on a live stream (mmi_lm_enable_adapters before mmi_batcher_create)");
        if (adapter_slot < -1 || adapter_slot >= S) return mmi_fail(MMI_ERR_INVALID, "mmi_lm_set_row_adapter: slot must be -1 (none) or in [0, max_adapters)");
    }
    if (settings && (rc = mmi_row_sampling_check(settings))) return rc;
    if (cond) {     // what mmi_lm_set_row_condition would refuse at the step, refused now: no slot is claimed
        if (!std::isfinite(cond->cfg_coef)) return mmi_fail(MMI_ERR_INVALID, "cfg_coef must be finite");
        if (cond->cfg_coef != 1.f && !b->guided) return mmi_fail(MMI_ERR_STATE, "cfg_coef != 1 needs a batcher created with guidance");
        if (cond->condition_sum && !b->has_sum) return mmi_fail(MMI_ERR_STATE, "the batcher was created without a sum condition");
        if (cond->condition_cross && !b->has_cross)
            return mmi_fail(MMI_ERR_INVALID, "a cross-attention condition was given to a model without cross-attention layers");
        if (cond->condition_cross && (cond->cross_len < 1 || cond->cross_len > b->cross_cap))
            return mmi_fail(MMI_ERR_SHAPE, "cross_len outside [1, capacity] (mmi_lm_set_cross_capacity before mmi_batcher_create)");
    }
    std::lock_guard<std::mutex> g(b->mu);
    for (auto& c : b->channels) {
        if (c.live) continue;
        c = Channel();
        c.live = true;
        c.pending_reset = true;
        if (settings) { c.own_sampling = true; c.sampling = *settings; }
        c.adapter = adapter_slot;
        if (cond) {
            c.own_cond = true;
            c.coef = cond->cfg_coef;
            const size_t D = (size_t)b->dim;
            if (cond->condition_sum) {
                const uint16_t* p = reinterpret_cast<const uint16_t*>(cond->condition_sum);
                c.cond_sum.assign(p, p + b->R * D);
            }
            if (cond->condition_cross) {
                const uint16_t* p = reinterpret_cast<const uint16_t*>(cond->condition_cross);
                c.cross_len = cond->cross_len;
                c.cond_cross.assign(p, p + (size_t)b->R * c.cross_len * D);
            }
        }
        c.id = b->next_id++;
        *channel_id = c.id;
        b->stats.used_slots += 1;
        return MMI_OK;
    }
    return mmi_fail(MMI_ERR_BUSY, "no free slot");   // py_module.rs:443-470: `channels()` yields None
}

// A live channel duplicated into a free slot.  No reference counterpart: batched_asr.rs opens a slot fresh; the
// nearest is get_streaming_state / set_streaming_state on a batch of one (streaming.py:158-181).  Both engine forks run on the
// batcher's stream, so they are ordered behind the last step and in front of the next one.
extern "C" int mmi_batcher_fork(mmi_batcher* b, int64_t parent_channel, const mmi_row_sampling* settings, int64_t* channel_id) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b || !channel_id) return mmi_fail(MMI_ERR_INVALID, "null argument");
    int rc;
    if (settings && (rc = mmi_row_sampling_check(settings))) return rc;
    std::lock_guard<std::mutex> step_guard(b->step_mu);
    std::lock_guard<std::mutex> g(b->mu);
    Channel* parent = find_channel(b, parent_channel);
    if (!parent) return mmi_fail(MMI_ERR_NO_CHANNEL, "unknown channel");
    if (parent->pending_reset) return mmi_fail(MMI_ERR_STATE, "mmi_batcher_fork: the parent was opened since the last step: it has no state yet");
    const int src = (int)(parent - b->channels.data());
    int32_t dst = -1;
    for (int r = 0; r < b->B && dst < 0; ++r)
        if (!b->channels[r].live) dst = r;
    if (dst < 0) return mmi_fail(MMI_ERR_BUSY, "no free slot");
    if ((rc = mmi_mimi_fork_session(b->mimi, src, &dst, 1, b->stream))) return rc;
    if ((rc = mmi_lm_fork_session(b->lm, src, &dst, 1, b->stream))) return rc;
    if (settings) {
        std::vector<uint8_t> mask((size_t)b->B, 0);
        std::vector<mmi_row_sampling> rows((size_t)b->B, *settings);
        mask[dst] = 1;
        if ((rc = mmi_lm_set_row_sampling(b->lm, mask.data(), rows.data(), b->stream))) return rc;
    }
    Channel& c = b->channels[dst];
    c = Channel();
    c.live = true;
    c.own_sampling = settings ? true : parent->own_sampling;
    c.sampling = settings ? *settings : parent->sampling;
    c.own_cond = parent->own_cond; c.coef = parent->coef; c.cross_len = parent->cross_len;
    c.adapter = parent->adapter;
    c.own_top_p = parent->own_top_p; c.top_p_dirty = parent->top_p_dirty; c.top_p = parent->top_p; c.top_p_text = parent->top_p_text;
    c.frames = parent->frames;
    // the rows' mirrors follow the engine: the child's rows hold what the parent's hold
    b->row_has_cond[dst] = b->row_has_cond[src];
    b->row_adapter[dst] = b->row_adapter[src];
    b->row_has_top_p[dst] = b->row_has_top_p[src];
    c.id = b->next_id++;
    *channel_id = c.id;
    b->stats.used_slots += 1;
    return MMI_OK;
}

int32_t mmi_lm_nucleus_enabled(const mmi_lm* lm);

extern "C" int mmi_batcher_set_channel_top_p(mmi_batcher* b, int64_t channel_id, float top_p, float top_p_text) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b) return mmi_fail(MMI_ERR_INVALID, "null handle");
    // what mmi_lm_set_row_top_p would refuse at the step, refused now
    if (mmi_lm_nucleus_enabled(b->lm) <= 0) return mmi_fail(MMI_ERR_STATE, "the stream was started without the nucleus samplers (mmi_lm_enable_nucleus before mmi_batcher_create)");
    for (float v : {top_p, top_p_text})
        if (!std::isfinite(v) || v < 0.f || v > 1.f) return mmi_fail(MMI_ERR_INVALID, "top_p and top_p_text must lie in [0, 1] (0 = off)");
    std::lock_guard<std::mutex> g(b->mu);
    Channel* c = find_channel(b, channel_id);
    if (!c) return mmi_fail(MMI_ERR_NO_CHANNEL, "unknown channel");
    c->own_top_p = c->top_p_dirty = true;
    c->top_p = top_p;
    c->top_p_text = top_p_text;
    return MMI_OK;
}

extern "C" int mmi_batcher_close(mmi_batcher* b, int64_t channel_id) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b) return mmi_fail(MMI_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> g(b->mu);
    Channel* c = find_channel(b, channel_id);
    if (!c) return mmi_fail(MMI_ERR_NO_CHANNEL, "unknown channel");
    *c = Channel();
    b->stats.used_slots -= 1;
    return MMI_OK;
}

extern "C" int mmi_batcher_push_pcm(mmi_batcher* b, int64_t channel_id, const float* pcm, int32_t n_samples) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b || (!pcm && n_samples > 0) || n_samples < 0) return mmi_fail(MMI_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> g(b->mu);
    Channel* c = find_channel(b, channel_id);
    if (!c) return mmi_fail(MMI_ERR_NO_CHANNEL, "unknown channel");
    if (c->in.size() + (size_t)n_samples > (size_t)b->cfg.max_buffered_frames * b->F)
        return mmi_fail(MMI_ERR_BUSY, "channel input buffer full");
    c->in.insert(c->in.end(), pcm, pcm + n_samples);
    return MMI_OK;
}

extern "C" int mmi_batcher_step(mmi_batcher* b, int32_t* n_active) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b) return mmi_fail(MMI_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> step_guard(b->step_mu);
    const int B = b->B, F = b->F;
    Staging& h = b->host;
    Staging& d = b->dev;
    int active = 0, resets = 0, firsts = 0, sets = 0, adapts = 0, tops = 0;
    {   // ---- pre_process (batched_asr.rs:279-374)
        std::lock_guard<std::mutex> g(b->mu);
        for (int r = 0; r < B; ++r) {
            Channel& c = b->channels[r];
            h.exec[r] = h.first[r] = h.reset[r] = 0;
            b->row_owner[r] = c.live ? c.id : 0;
            float* dst = h.pcm + (size_t)r * F;
            {   // the row's adapter follows its channel: the owner's for the channel's life, none once it is closed
                const int want = c.live ? c.adapter : -1;
                b->adapter_plan[r] = want != b->row_adapter[r] ? want : -2;
                if (b->adapter_plan[r] != -2) ++adapts;
            }
            {   // and so does its top_p: the owner's for the channel's life, the handle's again at the step after close
                mmi_batcher::TopPPlan& tp = b->top_p_plan[r];
                tp.what = 0;
                if (c.live && c.own_top_p && c.top_p_dirty) tp = mmi_batcher::TopPPlan{1, c.top_p, c.top_p_text};
                else if (!(c.live && c.own_top_p) && b->row_has_top_p[r]) tp.what = 2;
                if (tp.what) ++tops;
            }
            if (c.live && c.pending_reset) {
                h.reset[r] = 1;
                c.pending_reset = false;
                ++resets;
                b->m_set[r] = c.own_sampling ? 1 : 0;
                b->m_clear[r] = c.own_sampling ? 0 : 1;
                if (c.own_sampling) { b->row_set[r] = c.sampling; ++sets; }
                mmi_batcher::CondPlan& cp = b->cond_plan[r];
                cp.what = c.own_cond ? 1 : (b->row_has_cond[r] ? 2 : 0);
                cp.prev = b->row_has_cond[r] != 0;
                if (c.own_cond) {       // into the slot's pinned region (the last step's copy out of it has completed)
                    uint16_t* reg = b->h_cond ? b->h_cond + (size_t)r * b->cond_slot : nullptr;
                    cp.coef = c.coef; cp.sum = !c.cond_sum.empty(); cp.cross = !c.cond_cross.empty(); cp.len = c.cross_len;
                    if (cp.sum) std::copy(c.cond_sum.begin(), c.cond_sum.end(), reg);
                    if (cp.cross) std::copy(c.cond_cross.begin(), c.cond_cross.end(), reg + (size_t)b->R * b->dim);
                    c.cond_sum = std::vector<uint16_t>();
                    c.cond_cross = std::vector<uint16_t>();
                }
                b->row_has_cond[r] = c.own_cond ? 1 : 0;
            } else { b->m_set[r] = b->m_clear[r] = 0; b->cond_plan[r].what = 0; }
            if (c.live && c.in.size() >= (size_t)F) {
                std::copy(c.in.begin(), c.in.begin() + F, dst);
                c.in.erase(c.in.begin(), c.in.begin() + F);
                h.exec[r] = 1;
                if (c.frames == 0 && b->cfg.reset_codec_after_first_frame) {
                    h.first[r] = 1;
                    ++firsts;
                }
                c.frames += 1;
                ++active;
            } else {
                memset(dst, 0, (size_t)F * sizeof(float));
            }
        }
    }
    if (n_active) *n_active = active;
    if (active == 0 && resets == 0 && adapts == 0 && tops == 0) return MMI_OK;
    hipStream_t s = b->stream;
    int rc;
    MMI_HIP_CHECK(hipEventRecord(b->ev_begin, s));
    MMI_HIP_CHECK(hipMemcpyAsync(d.up, h.up, h.h2d_bytes, hipMemcpyHostToDevice, s));
    for (int r = 0; adapts && r < B; ++r) {      // the mirror follows the engine: a failed step leaves the change to be made again
        if (b->adapter_plan[r] == -2) continue;
        if ((rc = mmi_lm_set_row_adapter(b->lm, r, b->adapter_plan[r], s))) return rc;
        b->row_adapter[r] = b->adapter_plan[r];
    }
    for (int r = 0; tops && r < B; ++r) {
        const mmi_batcher::TopPPlan& tp = b->top_p_plan[r];
        if (!tp.what) continue;
        if ((rc = tp.what == 1 ? mmi_lm_set_row_top_p(b->lm, r, tp.top_p, tp.top_p_text, s) : mmi_lm_clear_row_top_p(b->lm, r, s))) return rc;
        b->row_has_top_p[r] = tp.what == 1 ? 1 : 0;
        if (tp.what == 1) {
            std::lock_guard<std::mutex> g(b->mu);
            Channel& c = b->channels[r];
            if (c.live && c.id == b->row_owner[r] && c.top_p == tp.top_p && c.top_p_text == tp.top_p_text) c.top_p_dirty = false;
        }
    }
    if (resets) {   // handle_chat: mimi.reset_streaming(); lm_gen.reset_streaming() (server.py:163-164), for the new rows only
        if ((rc = mmi_mimi_reset(b->mimi, d.reset, s))) return rc;
        if ((rc = mmi_lm_reset(b->lm, d.reset, s))) return rc;
        // the new owner's sampling settings: its own (open_with), or the batcher's again whatever the slot's last owner had
        if (resets > sets && (rc = mmi_lm_clear_row_sampling(b->lm, b->m_clear.data(), s))) return rc;
        if (sets && (rc = mmi_lm_set_row_sampling(b->lm, b->m_set.data(), b->row_set.data(), s))) return rc;
        // the new owner's condition: its own (open_cond), or cfg.guidance's again if the slot's last owner had one
        for (int r = 0; r < B; ++r) {
            const mmi_batcher::CondPlan& cp = b->cond_plan[r];
            if (!cp.what) continue;
            const size_t off = (size_t)r * b->cond_slot, sum_n = (size_t)b->R * b->dim;
            mmi_row_condition rc_;
            if (cp.what == 1) {
                const size_t n = cp.cross ? sum_n + (size_t)b->R * cp.len * b->dim : (cp.sum ? sum_n : 0);
                if (n) MMI_HIP_CHECK(hipMemcpyAsync(b->d_cond + off, b->h_cond + off, n * sizeof(uint16_t), hipMemcpyHostToDevice, s));
                rc_.cfg_coef = cp.coef;
                // a part the channel does not bring is cfg.guidance's: kept, or given back if the slot's last owner had replaced it
                rc_.condition_sum = cp.sum ? b->d_cond + off : (cp.prev && b->has_sum ? b->d_def + off : nullptr);
                rc_.condition_cross = cp.cross ? b->d_cond + off + sum_n : (cp.prev && b->has_cross ? b->d_def + off + sum_n : nullptr);
                rc_.cross_len = cp.cross ? cp.len : b->cross_len0;
            } else {
                rc_.cfg_coef = b->coef0;
                rc_.condition_sum = b->has_sum ? b->d_def + off : nullptr;
                rc_.condition_cross = b->has_cross ? b->d_def + off + sum_n : nullptr;
                rc_.cross_len = b->cross_len0;
            }
            if ((rc = mmi_lm_set_row_condition(b->lm, r, &rc_, s))) return rc;
        }
    }
    if (active == 0) {
        MMI_HIP_CHECK(hipStreamSynchronize(s));
        return MMI_OK;
    }
    // ---- the frame step with the stream mask (batched_asr.rs:233-262; server.py:132-146)
    if ((rc = mmi_mimi_set_exec_mask(b->mimi, d.exec, s))) return rc;
    if ((rc = mmi_lm_set_exec_mask(b->lm, d.exec, s))) return rc;
    if ((rc = mmi_mimi_encode_step(b->mimi, d.pcm, b->d_codes, B, 1, s))) return rc;
    if (firsts && (rc = mmi_mimi_reset(b->mimi, d.first, s))) return rc;   // server.py:135-141
    int valid = 0;
    if ((rc = mmi_lm_step(b->lm, b->d_codes, b->K, d.tokens, nullptr, nullptr, nullptr, B, &valid, s))) return rc;
    if (b->lp_on) {       // the frame's log-probabilities, lined up with d.tokens
        const size_t n = (size_t)B * b->NTOK;
        if ((rc = mmi_lm_frame_logprobs(b->lm, b->d_lp, b->d_lp_id, b->d_lp_top, s))) return rc;
        MMI_HIP_CHECK(hipMemcpyAsync(b->h_lp, b->d_lp, n * sizeof(float), hipMemcpyDeviceToHost, s));
        if (b->lp_top_n) {
            MMI_HIP_CHECK(hipMemcpyAsync(b->h_lp_id, b->d_lp_id, n * b->lp_top_n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            MMI_HIP_CHECK(hipMemcpyAsync(b->h_lp_top, b->d_lp_top, n * b->lp_top_n * sizeof(float), hipMemcpyDeviceToHost, s));
        }
    }
    MMI_LAUNCH(k_batcher_route, mmi_cdiv(B, 64), 64, 0, s, (const long*)d.tokens, (const uint8_t*)d.exec, d.played,
               (long*)b->d_dec_codes, B, b->dep_q, b->card);
    MMI_CHECK_LAUNCH();
    if (b->dep_q > 0) {   // an ASR-style model (dep_q = 0) generates no audio: the step ends at the text token
        if ((rc = mmi_mimi_set_exec_mask(b->mimi, d.played, s))) return rc;   // rows still inside the LM delay do not touch the decoder
        if ((rc = mmi_mimi_decode_step(b->mimi, b->d_dec_codes, d.pcm_out, B, b->dep_q, 1, s))) return rc;
    }
    MMI_HIP_CHECK(hipMemcpyAsync(h.down, d.down, h.d2h_bytes, hipMemcpyDeviceToHost, s));
    MMI_HIP_CHECK(hipEventRecord(b->ev_end, s));
    MMI_HIP_CHECK(hipEventSynchronize(b->ev_end));
    float ms = 0.f;
    hipEventElapsedTime(&ms, b->ev_begin, b->ev_end);
    {   // ---- post_process (batched_asr.rs:376-437): a row's result goes to the channel that owned the row at pre_process
        std::lock_guard<std::mutex> g(b->mu);
        b->stats.steps += 1;
        b->stats.frames += active;
        b->stats.last_step_ms = ms;
        for (int r = 0; r < B; ++r) {
            if (!h.exec[r] || !h.played[r]) continue;
            Channel& c = b->channels[r];
            if (!c.live || c.id != b->row_owner[r]) continue;   // closed (or re-opened by someone else) meanwhile
            if ((int)c.out.size() >= b->cfg.max_buffered_frames) {
                c.out.pop_front();
                b->stats.dropped_frames += 1;
            }
            OutFrame f;
            f.pcm.assign(h.pcm_out + (size_t)r * F, h.pcm_out + (size_t)(r + 1) * F);
            f.tokens.assign(h.tokens + (size_t)r * b->NTOK, h.tokens + (size_t)(r + 1) * b->NTOK);
            if (b->lp_on) {
                const size_t n = (size_t)b->NTOK, m = n * b->lp_top_n;
                f.logp.assign(b->h_lp + r * n, b->h_lp + (r + 1) * n);
                if (m) {
                    f.top_id.assign(b->h_lp_id + r * m, b->h_lp_id + (r + 1) * m);
                    f.top_logp.assign(b->h_lp_top + r * m, b->h_lp_top + (r + 1) * m);
                }
            }
            c.out.push_back(std::move(f));
        }
    }
    return MMI_OK;
}

static int pop_frame(mmi_batcher* b, int64_t channel_id, float* pcm, int64_t* tokens, float* logp, int32_t* top_id, float* top_logp, int32_t* got);

extern "C" int mmi_batcher_pop(mmi_batcher* b, int64_t channel_id, float* pcm, int64_t* tokens, int32_t* got) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b || !got) return mmi_fail(MMI_ERR_INVALID, "null argument");
    return pop_frame(b, channel_id, pcm, tokens, nullptr, nullptr, nullptr, got);
}

extern "C" int mmi_batcher_pop_logprobs(mmi_batcher* b, int64_t channel_id, float* pcm, int64_t* tokens, float* logp, int32_t* top_id,
                                        float* top_logp, int32_t* got) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b || !got) return mmi_fail(MMI_ERR_INVALID, "null argument");
    if (!logp) return mmi_fail(MMI_ERR_INVALID, "mmi_batcher_pop_logprobs: logp must not be null");
    if (!b->lp_on) return mmi_fail(MMI_ERR_STATE, "mmi_batcher_pop_logprobs: log-probabilities are not enabled (mmi_lm_enable_logprobs before mmi_batcher_create)");
    if ((top_id || top_logp) && b->lp_top_n == 0)
        return mmi_fail(MMI_ERR_INVALID, "mmi_batcher_pop_logprobs: the handle records no alternatives (top_n == 0)");
    return pop_frame(b, channel_id, pcm, tokens, logp, top_id, top_logp, got);
}

static int pop_frame(mmi_batcher* b, int64_t channel_id, float* pcm, int64_t* tokens, float* logp, int32_t* top_id, float* top_logp, int32_t* got) {
    std::lock_guard<std::mutex> g(b->mu);
    Channel* c = find_channel(b, channel_id);
    if (!c) return mmi_fail(MMI_ERR_NO_CHANNEL, "unknown channel");
    *got = 0;
    if (c->out.empty()) return MMI_OK;
    OutFrame& f = c->out.front();
    if (pcm) std::copy(f.pcm.begin(), f.pcm.end(), pcm);
    if (tokens) std::copy(f.tokens.begin(), f.tokens.end(), tokens);
    if (logp) std::copy(f.logp.begin(), f.logp.end(), logp);
    if (top_id) std::copy(f.top_id.begin(), f.top_id.end(), top_id);
    if (top_logp) std::copy(f.top_logp.begin(), f.top_logp.end(), top_logp);
    c->out.pop_front();
    *got = 1;
    return MMI_OK;
}

extern "C" int mmi_batcher_get_stats(mmi_batcher* b, mmi_batcher_stats* out) {
    MmiDeviceGuard dev_guard_(b ? mmi_lm_device(b->lm) : -1);
    if (!b || !out) return mmi_fail(MMI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    *out = b->stats;
    return MMI_OK;
}
