// A Python-free self-test of an installed libmoshi_mi.so on a GPU box: a tiny Mimi and a tiny Moshi LM are built through the C ABI
// (include/moshi_mi.h) from weights this program generates itself (an integer hash, the same one
// tests/golden/make_native_selftest.py uses), run for a few frames, and compared with what the numpy oracle computed for them
// (tests/golden/native_selftest/expected.bin): RVQ codes and teacher-forced token-ring outputs bit-exact, PCM within 2e-5, logits
// within the bf16 tolerance of tests/lm_cases.py (5 % max / 1.2 % mean of max|logit| per row and site).  ~1 s, no torch.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -Iinclude scripts/native_selftest.cpp -Lmoshi_amd -lmoshi_mi \
//         -Wl,-rpath,'$ORIGIN/../moshi_amd' -o build/native_selftest && build/native_selftest tests/golden/native_selftest
//
// `native_selftest <dir> --rows 65,128`: the LM alone on handles of that many model rows (mmi_lm_create_rows, the many-row GEMM): row r
// replays the fixture's session r % B against the same recorded values, and a snapshot taken mid-stream resumes bit for bit.
//
// `native_selftest <dir> --adapters`: the LM alone on an adapter handle (mmi_lm_enable_adapters): enable, load an adapter
// this program generates, every row without an adapter against the recorded values, one row on the adapter (it alone changes),
// the refusals while the row is live, unload, destroy.
//
// `native_selftest <dir> --nucleus`: the LM alone with the nucleus samplers (mmi_lm_enable_nucleus): a free-running
// sampling stream with top_p = top_p_text = 1e-6 must equal the greedy stream (the nucleus is the argmax alone), and the entry points'
// refusals must hold.
//
// `native_selftest <dir> --prefill`: chunked prefill through the C ABI alone (mmi_lm_enable_prefill / mmi_lm_prefill): the
// first recorded forced frames enter the sessions by prefill - on a handle of the fixture's batch in one pass and in passes of one
// frame, and on a 128-row handle whose 66 sessions make every pass a k_gemm_rows launch - then the remaining frames are stepped
// against the oracle's record; the entry points' refusals must hold.
//
// `native_selftest <dir> --score`: teacher-forced scoring through the C ABI alone (mmi_lm_enable_score / mmi_lm_score): the
// first recorded forced frames go through mmi_lm_score with commit = 1 - in one pass and in passes of one frame - the returned logits
// against the recorded step logits, logp against the double-precision value from the returned logits; the remaining frames are then
// stepped against the record; the entry points' refusals must hold.
//
// The same source builds against the CPU simulator (-DMMI_SELFTEST_SIM, tests/test_native_selftest.py), which is how the expected
// values and this program are checked where there is no GPU.  The checker side (oracle) never runs here: only its recorded output.
//
// The sanitizer run (host code only: the engine and its kernels compiled for the simulator into ONE program with this main, no
// LD_PRELOAD, no GPU); both modes must end in SELFTEST PASSED with no report:
//
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -pthread -w -fsanitize=address,undefined -fno-omit-frame-pointer \
//         -DHIPSIM_UCONTEXT -DMMI_SELFTEST_SIM -Itests/hipsim -Imoshi_amd/csrc -Iinclude -x c++ \
//         moshi_amd/csrc/{api_common,mimi_engine,lm_engine,batcher,duplex}.hip tests/hipsim/hipsim.cpp scripts/native_selftest.cpp \
//         -o build/native_selftest_san
//   export MMI_NO_GRAPH=1 ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 UBSAN_OPTIONS=print_stacktrace=1
//   build/native_selftest_san tests/golden/native_selftest && build/native_selftest_san tests/golden/native_selftest --rows 65,128 &&
//   build/native_selftest_san tests/golden/native_selftest --adapters && build/native_selftest_san tests/golden/native_selftest --nucleus &&
//   build/native_selftest_san tests/golden/native_selftest --prefill && build/native_selftest_san tests/golden/native_selftest --score
#include "moshi_mi.h"
#ifdef MMI_SELFTEST_SIM
#include "hipsim.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#define HCK(x) do { if ((x) != hipSuccess) { printf("HIP call failed at line %d\n", __LINE__); exit(2); } } while (0)
#define MCK(x) do { int rc_ = (x); if (rc_) { printf("%s -> %d: %s\n", #x, rc_, mmi_last_error()); exit(3); } } while (0)

static float u_of(uint32_t seed, uint32_t i) {
    uint32_t h = (i * 2654435761u) ^ seed;
    h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
    return (float)((int)(h & 0xffffu) - 32768) * (1.0f / 32768.0f);
}
static uint16_t bf16_rne(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}

struct Tensor { std::string model, name; int bf16, ndim; long d[4]; float base, scale; uint32_t seed; void* dev = nullptr; };
struct Expected { std::string name; int i64; long count, off; };

int main(int argc, char** argv) {
    const std::string dir = argc > 1 && strncmp(argv[1], "--", 2) ? argv[1] : "tests/golden/native_selftest";
    // --rows N[,N...]: instead of the codec + LM pass, the LM alone on handles of N model rows made by mmi_lm_create_rows (65..128:
    // the many-row GEMM).  Row r replays the fixture's session r % B - rows never mix, so its ring outputs and
    // logits are the oracle's recorded ones - then a snapshot taken mid-stream must resume bit for bit.
    std::vector<int> many_rows;
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--rows"))
            for (const char* q = argv[i + 1]; *q; q = strchr(q, ',') ? strchr(q, ',') + 1 : q + strlen(q)) many_rows.push_back(atoi(q));
    bool adapters = false;
    for (int i = 1; i < argc; ++i) adapters |= !strcmp(argv[i], "--adapters");
    bool nucleus = false;
    for (int i = 1; i < argc; ++i) nucleus |= !strcmp(argv[i], "--nucleus");
    bool prefill = false;
    for (int i = 1; i < argc; ++i) prefill |= !strcmp(argv[i], "--prefill");
    bool score = false;
    for (int i = 1; i < argc; ++i) score |= !strcmp(argv[i], "--score");
    FILE* mf = fopen((dir + "/manifest.txt").c_str(), "r");
    if (!mf) { printf("cannot open %s/manifest.txt\n", dir.c_str()); return 2; }
    mmi_mimi_cfg mc; mmi_lm_cfg lc;
    memset(&mc, 0, sizeof(mc)); memset(&lc, 0, sizeof(lc));
    std::vector<Tensor> tensors; std::vector<Expected> exps;
    int B = 0, FR = 0, K = 0, ST = 0, fs = 0, n_user = 0, dep_q = 0, card = 0, text_card = 0;
    char tag[64];
    while (fscanf(mf, "%63s", tag) == 1) {
        if (!strcmp(tag, "mimi_cfg")) {
            int32_t* p = (int32_t*)&mc;            // header order: 6 ints, ratios[8], 10 ints, 1 float, 4 ints
            for (int i = 0; i < 6 + 8 + 10; ++i) if (fscanf(mf, "%d", p + i) != 1) return 2;
            if (fscanf(mf, "%f", &mc.tr_max_period) != 1) return 2;
            if (fscanf(mf, "%d %d %d %d", &mc.q_dimension, &mc.q_bins, &mc.q_n_q, &mc.q_n_q_semantic) != 4) return 2;
        } else if (!strcmp(tag, "lm_cfg")) {
            if (fscanf(mf, "%d %d %d %d %d %f", &lc.dim, &lc.num_heads, &lc.num_layers, &lc.ffn_hidden, &lc.context, &lc.max_period) != 6) return 2;
            if (fscanf(mf, "%d %d %d %d %d %d %d %d %d", &lc.n_q, &lc.dep_q, &lc.card, &lc.text_card, &lc.text_card_out, &lc.depformer_dim,
                       &lc.depformer_num_heads, &lc.depformer_num_layers, &lc.depformer_ffn_hidden) != 9) return 2;
            for (int i = 0; i < 64; ++i) if (fscanf(mf, "%d", &lc.delays[i]) != 1) return 2;
            if (fscanf(mf, "%d %d %d %d %d", &lc.existing_text_padding_id, &lc.extra_heads_num_heads, &lc.extra_heads_dim, &lc.kv_cache_dtype,
                       &lc.cross_attention) != 5) return 2;
        } else if (!strcmp(tag, "T")) {
            Tensor t; char model[16], name[256], dt[8], b[64], s[64];
            if (fscanf(mf, "%15s %255s %7s %d %ld %ld %ld %ld %63s %63s %u", model, name, dt, &t.ndim, &t.d[0], &t.d[1], &t.d[2], &t.d[3], b, s, &t.seed) != 11) return 2;
            t.model = model; t.name = name; t.bf16 = !strcmp(dt, "bf16"); t.base = strtof(b, nullptr); t.scale = strtof(s, nullptr);
            tensors.push_back(t);
        } else if (!strcmp(tag, "run")) {
            if (fscanf(mf, "%d %d %d %d %d %d %d %d %d", &B, &FR, &K, &ST, &fs, &n_user, &dep_q, &card, &text_card) != 9) return 2;
        } else if (!strcmp(tag, "E")) {
            Expected e; char name[64], dt[8];
            if (fscanf(mf, "%63s %7s %ld %ld", name, dt, &e.count, &e.off) != 4) return 2;
            e.name = name; e.i64 = !strcmp(dt, "i64");
            exps.push_back(e);
        } else { printf("manifest: unknown line '%s'\n", tag); return 2; }
    }
    fclose(mf);
    std::vector<unsigned char> blob;
    {
        FILE* bf = fopen((dir + "/expected.bin").c_str(), "rb");
        if (!bf) { printf("cannot open expected.bin\n"); return 2; }
        fseek(bf, 0, SEEK_END); long n = ftell(bf); fseek(bf, 0, SEEK_SET);
        blob.resize(n);
        if (fread(blob.data(), 1, n, bf) != (size_t)n) return 2;
        fclose(bf);
    }
    auto expect = [&](const char* name) -> const void* {
        for (auto& e : exps) if (e.name == name) return blob.data() + e.off;
        printf("expected.bin has no %s\n", name); exit(2);
    };
    printf("libmoshi_mi ABI version %d; %zu tensors; B=%d frames=%d K=%d steps=%d\n", mmi_version(), tensors.size(), B, FR, K, ST);

    // ---- weights: generated here, uploaded, described by the reference's state-dict names
    std::vector<mmi_tensor_desc> md, ld;
    for (auto& t : tensors) {
        long n = 1; for (int i = 0; i < t.ndim; ++i) n *= t.d[i];
        std::vector<float> v(n);
        for (long i = 0; i < n; ++i) { const float x = t.scale * u_of(t.seed, (uint32_t)i); v[i] = t.base + x; }
        const size_t bytes = (size_t)n * (t.bf16 ? 2 : 4);
        HCK(hipMalloc(&t.dev, bytes));
        if (t.bf16) {
            std::vector<uint16_t> h(n);
            for (long i = 0; i < n; ++i) h[i] = bf16_rne(v[i]);
            HCK(hipMemcpy(t.dev, h.data(), bytes, hipMemcpyHostToDevice));
        } else HCK(hipMemcpy(t.dev, v.data(), bytes, hipMemcpyHostToDevice));
        mmi_tensor_desc d; memset(&d, 0, sizeof(d));
        d.name = t.name.c_str(); d.data = t.dev; d.dtype = t.bf16 ? MMI_BF16 : MMI_F32; d.ndim = t.ndim;
        for (int i = 0; i < 4; ++i) d.shape[i] = i < t.ndim ? t.d[i] : 0;
        (t.model == "mimi" ? md : ld).push_back(d);
    }
    int failures = 0;

    // ---- Mimi: encode FR frames, decode the oracle's codes
    if (many_rows.empty() && !adapters && !nucleus && !prefill && !score) {
        mmi_mimi* m = nullptr;
        MCK(mmi_mimi_create(&mc, md.data(), (int32_t)md.size(), B, &m));
        MCK(mmi_mimi_set_num_codebooks(m, K));
        MCK(mmi_mimi_streaming_start(m, B, nullptr));
        const int64_t* ecodes = (const int64_t*)expect("mimi_codes");
        const float* epcm = (const float*)expect("mimi_pcm");
        float *dx, *dpcm; int64_t *dc, *dcin;
        HCK(hipMalloc((void**)&dx, (size_t)B * fs * 4)); HCK(hipMalloc((void**)&dpcm, (size_t)B * fs * 4));
        HCK(hipMalloc((void**)&dc, (size_t)B * K * 8)); HCK(hipMalloc((void**)&dcin, (size_t)B * K * 8));
        long code_diffs = 0; double worst_pcm = 0;
        for (int f = 0; f < FR; ++f) {
            std::vector<float> x((size_t)B * fs);
            for (size_t i = 0; i < x.size(); ++i) x[i] = 0.3f * u_of(77u + f, (uint32_t)i);
            HCK(hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice));
            MCK(mmi_mimi_encode_step(m, dx, dc, B, 1, nullptr));
            HCK(hipMemcpy(dcin, ecodes + (size_t)f * B * K, (size_t)B * K * 8, hipMemcpyHostToDevice));
            MCK(mmi_mimi_decode_step(m, dcin, dpcm, B, K, 1, nullptr));
            HCK(hipDeviceSynchronize());
            std::vector<int64_t> c((size_t)B * K); std::vector<float> p((size_t)B * fs);
            HCK(hipMemcpy(c.data(), dc, c.size() * 8, hipMemcpyDeviceToHost));
            HCK(hipMemcpy(p.data(), dpcm, p.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < c.size(); ++i) code_diffs += c[i] != ecodes[(size_t)f * B * K + i];
            for (int b = 0; b < B; ++b) {
                double mx = 0, d = 0;
                for (int i = 0; i < fs; ++i) {
                    const float r = epcm[((size_t)f * B + b) * fs + i];
                    mx = fmax(mx, fabs(r)); d = fmax(d, fabs(p[(size_t)b * fs + i] - r));
                }
                worst_pcm = fmax(worst_pcm, d / (2e-5 + 2e-5 * mx));
            }
        }
        printf("mimi: %ld of %d code indices differ from the oracle (must be 0); worst PCM error %.3f of its tolerance (must be <= 1)\n",
               code_diffs, FR * B * K, worst_pcm);
        failures += code_diffs != 0 || !(worst_pcm <= 1.0);
        MCK(mmi_mimi_streaming_stop(m));
        mmi_mimi_destroy(m);
    }
    // ---- LM: greedy steps, teacher-forced with the oracle's tokens
    if (many_rows.empty() && !adapters && !nucleus && !prefill && !score) {
        mmi_lm* lm = nullptr;
        MCK(mmi_lm_create(&lc, ld.data(), (int32_t)ld.size(), B, &lm));
        mmi_sampling sp; memset(&sp, 0, sizeof(sp));
        sp.use_sampling = 0; sp.temp = 0.8f; sp.temp_text = 0.7f; sp.top_k = 250; sp.top_k_text = 25; sp.seed = 0;
        MCK(mmi_lm_streaming_start(lm, B, &sp, nullptr));
        const int NT = dep_q + 1;
        const int64_t* eforced = (const int64_t*)expect("lm_forced");
        const int64_t* eout = (const int64_t*)expect("lm_out");
        const float* etl = (const float*)expect("lm_text_logits");
        const float* eal = (const float*)expect("lm_audio_logits");
        int64_t *duc, *dforced, *dout; float *dtl, *dal;
        HCK(hipMalloc((void**)&duc, (size_t)B * n_user * 8)); HCK(hipMalloc((void**)&dforced, (size_t)B * NT * 8));
        HCK(hipMalloc((void**)&dout, (size_t)B * NT * 8));
        HCK(hipMalloc((void**)&dtl, (size_t)B * text_card * 4)); HCK(hipMalloc((void**)&dal, (size_t)B * dep_q * card * 4));
        long tok_diffs = 0; double worst_max = 0, worst_mean = 0;
        auto site = [&](const float* a, const float* r, int n) {
            double mx = 1e-6, dmax = 0, dsum = 0;
            for (int i = 0; i < n; ++i) { mx = fmax(mx, fabs(r[i])); const double d = fabs(a[i] - r[i]); dmax = fmax(dmax, d); dsum += d; }
            worst_max = fmax(worst_max, dmax / mx); worst_mean = fmax(worst_mean, dsum / n / mx);
        };
        for (int s = 0; s < ST; ++s) {
            std::vector<int64_t> uc((size_t)B * n_user);
            for (size_t i = 0; i < uc.size(); ++i) uc[i] = (int64_t)((u_of(9000u + s, (uint32_t)i) + 1.0f) * 32768.0f) % card;
            HCK(hipMemcpy(duc, uc.data(), uc.size() * 8, hipMemcpyHostToDevice));
            HCK(hipMemcpy(dforced, eforced + (size_t)s * B * NT, (size_t)B * NT * 8, hipMemcpyHostToDevice));
            MCK(mmi_lm_force_next_tokens(lm, dforced, nullptr));
            int32_t valid = 0;
            MCK(mmi_lm_step(lm, duc, n_user, dout, dtl, dal, nullptr, B, &valid, nullptr));
            HCK(hipDeviceSynchronize());
            std::vector<int64_t> o((size_t)B * NT); std::vector<float> tl((size_t)B * text_card), al((size_t)B * dep_q * card);
            HCK(hipMemcpy(o.data(), dout, o.size() * 8, hipMemcpyDeviceToHost));
            HCK(hipMemcpy(tl.data(), dtl, tl.size() * 4, hipMemcpyDeviceToHost));
            HCK(hipMemcpy(al.data(), dal, al.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < o.size(); ++i) tok_diffs += o[i] != eout[(size_t)s * B * NT + i];
            for (int b = 0; b < B; ++b) {
                site(tl.data() + (size_t)b * text_card, etl + ((size_t)s * B + b) * text_card, text_card);
                for (int k = 0; k < dep_q; ++k) site(al.data() + ((size_t)b * dep_q + k) * card, eal + (((size_t)s * B + b) * dep_q + k) * card, card);
            }
        }
        printf("lm: %ld of %d token-ring outputs differ from the oracle (must be 0); logits worst max %.4f (<= 0.05), worst mean %.4f (<= 0.012) of max|logit|\n",
               tok_diffs, ST * B * NT, worst_max, worst_mean);
        failures += tok_diffs != 0 || !(worst_max <= 0.05) || !(worst_mean <= 0.012);
        MCK(mmi_lm_streaming_stop(lm));
        mmi_lm_destroy(lm);
    }
    for (int R : many_rows) {
        mmi_lm* lm = nullptr;
        MCK(mmi_lm_create_rows(&lc, nullptr, ld.data(), (int32_t)ld.size(), R, &lm));
        mmi_sampling sp; memset(&sp, 0, sizeof(sp));
        sp.use_sampling = 0; sp.temp = 0.8f; sp.temp_text = 0.7f; sp.top_k = 250; sp.top_k_text = 25; sp.seed = 0;
        MCK(mmi_lm_streaming_start(lm, R, &sp, nullptr));
        const int NT = dep_q + 1;
        const int64_t* eforced = (const int64_t*)expect("lm_forced");
        const int64_t* eout = (const int64_t*)expect("lm_out");
        const float* etl = (const float*)expect("lm_text_logits");
        const float* eal = (const float*)expect("lm_audio_logits");
        int64_t *duc, *dforced, *dout; float *dtl, *dal; void* dsnap;
        HCK(hipMalloc((void**)&duc, (size_t)R * n_user * 8)); HCK(hipMalloc((void**)&dforced, (size_t)R * NT * 8));
        HCK(hipMalloc((void**)&dout, (size_t)R * NT * 8));
        HCK(hipMalloc((void**)&dtl, (size_t)R * text_card * 4)); HCK(hipMalloc((void**)&dal, (size_t)R * dep_q * card * 4));
        const int64_t snap_bytes = mmi_lm_state_bytes(lm);
        HCK(hipMalloc(&dsnap, (size_t)snap_bytes));
        long tok_diffs = 0, snap_diffs = 0; double worst_max = 0, worst_mean = 0;
        auto site = [&](const float* a, const float* r, int n) {
            double mx = 1e-6, dmax = 0, dsum = 0;
            for (int i = 0; i < n; ++i) { mx = fmax(mx, fabs(r[i])); const double d = fabs(a[i] - r[i]); dmax = fmax(dmax, d); dsum += d; }
            worst_max = fmax(worst_max, dmax / mx); worst_mean = fmax(worst_mean, dsum / n / mx);
        };
        std::vector<int64_t> o((size_t)R * NT); std::vector<float> tl((size_t)R * text_card), al((size_t)R * dep_q * card);
        auto step = [&](int s) {
            std::vector<int64_t> uc1((size_t)B * n_user), uc((size_t)R * n_user), fo((size_t)R * NT);
            for (size_t i = 0; i < uc1.size(); ++i) uc1[i] = (int64_t)((u_of(9000u + s, (uint32_t)i) + 1.0f) * 32768.0f) % card;
            for (int r = 0; r < R; ++r) {
                memcpy(uc.data() + (size_t)r * n_user, uc1.data() + (size_t)(r % B) * n_user, (size_t)n_user * 8);
                memcpy(fo.data() + (size_t)r * NT, eforced + ((size_t)s * B + r % B) * NT, (size_t)NT * 8);
            }
            HCK(hipMemcpy(duc, uc.data(), uc.size() * 8, hipMemcpyHostToDevice));
            HCK(hipMemcpy(dforced, fo.data(), fo.size() * 8, hipMemcpyHostToDevice));
            MCK(mmi_lm_force_next_tokens(lm, dforced, nullptr));
            int32_t valid = 0;
            MCK(mmi_lm_step(lm, duc, n_user, dout, dtl, dal, nullptr, R, &valid, nullptr));
            HCK(hipDeviceSynchronize());
            HCK(hipMemcpy(o.data(), dout, o.size() * 8, hipMemcpyDeviceToHost));
            HCK(hipMemcpy(tl.data(), dtl, tl.size() * 4, hipMemcpyDeviceToHost));
            HCK(hipMemcpy(al.data(), dal, al.size() * 4, hipMemcpyDeviceToHost));
        };
        auto against_oracle = [&](int s) {
            for (int r = 0; r < R; ++r) {
                const int b = r % B;
                for (int i = 0; i < NT; ++i) tok_diffs += o[(size_t)r * NT + i] != eout[((size_t)s * B + b) * NT + i];
                site(tl.data() + (size_t)r * text_card, etl + ((size_t)s * B + b) * text_card, text_card);
                for (int k = 0; k < dep_q; ++k) site(al.data() + ((size_t)r * dep_q + k) * card, eal + (((size_t)s * B + b) * dep_q + k) * card, card);
            }
        };
        const int cut = ST / 2;
        int64_t host_word = 0;
        for (int s = 0; s < cut; ++s) { step(s); against_oracle(s); }
        MCK(mmi_lm_state_save(lm, dsnap, snap_bytes, &host_word, nullptr));
        std::vector<std::vector<int64_t>> first_o; std::vector<std::vector<float>> first_tl, first_al;
        for (int s = cut; s < ST; ++s) { step(s); against_oracle(s); first_o.push_back(o); first_tl.push_back(tl); first_al.push_back(al); }
        step(0);                                         // wander off
        MCK(mmi_lm_state_load(lm, dsnap, snap_bytes, host_word, nullptr));
        for (int s = cut; s < ST; ++s) {
            step(s);
            snap_diffs += o != first_o[s - cut] || memcmp(tl.data(), first_tl[s - cut].data(), tl.size() * 4) != 0 ||
                          memcmp(al.data(), first_al[s - cut].data(), al.size() * 4) != 0;
        }
        printf("lm %d rows (mmi_lm_create_rows, %lld k_gemm_rows launches): %ld of %d token-ring outputs differ from the oracle (must be 0); logits "
               "worst max %.4f (<= 0.05), worst mean %.4f (<= 0.012); %ld of %d steps differ after the snapshot (must be 0)\n",
               R, (long long)mmi_lm_stat(lm, 4), tok_diffs, ST * R * NT, worst_max, worst_mean, snap_diffs, ST - cut);
        failures += tok_diffs != 0 || !(worst_max <= 0.05) || !(worst_mean <= 0.012) || snap_diffs != 0 || (R > 64 && mmi_lm_stat(lm, 4) <= 0);
        MCK(mmi_lm_streaming_stop(lm));
        mmi_lm_destroy(lm);
        hipFree(duc); hipFree(dforced); hipFree(dout); hipFree(dtl); hipFree(dal); hipFree(dsnap);
    }
    if (adapters) {
        // every nn.Linear of the LM (the set the reference's replace_all_linear_with_lora wraps) gets lora_A [8, in], lora_B [out, 8]
        const int rank = 8;
        std::vector<std::string> names; std::vector<void*> bufs; std::vector<mmi_tensor_desc> ad;
        for (auto& t : tensors) {
            const std::string& n = t.name;
            const bool lin = t.model != "mimi" && t.ndim == 2 && n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0 &&
                             (n.find(".self_attn.in_projs.") != std::string::npos || n.find(".self_attn.out_projs.") != std::string::npos ||
                              n.find(".linear_in.weight") != std::string::npos || n.find(".linear_out.weight") != std::string::npos ||
                              n.compare(0, 13, "depformer_in.") == 0 || n.compare(0, 8, "linears.") == 0 || n == "text_linear.weight");
            if (!lin) continue;
            const std::string stem = n.substr(0, n.size() - 7);
            for (int which = 0; which < 2; ++which) {
                const long rows = which ? t.d[0] : rank, cols = which ? rank : t.d[1];
                std::vector<uint16_t> h((size_t)rows * cols);
                for (size_t i = 0; i < h.size(); ++i) h[i] = bf16_rne((which ? 0.25f : 2.0f / sqrtf((float)cols)) * u_of(t.seed + 17u + which, (uint32_t)i));
                void* dev; HCK(hipMalloc(&dev, h.size() * 2)); HCK(hipMemcpy(dev, h.data(), h.size() * 2, hipMemcpyHostToDevice));
                names.push_back(stem + (which ? ".lora_B.weight" : ".lora_A.weight")); bufs.push_back(dev);
                mmi_tensor_desc d; memset(&d, 0, sizeof(d));
                d.data = dev; d.dtype = MMI_BF16; d.ndim = 2; d.shape[0] = rows; d.shape[1] = cols;
                ad.push_back(d);
            }
        }
        for (size_t i = 0; i < ad.size(); ++i) ad[i].name = names[i].c_str();
        mmi_lm* lm = nullptr;
        MCK(mmi_lm_create(&lc, ld.data(), (int32_t)ld.size(), B, &lm));
        MCK(mmi_lm_enable_adapters(lm, 2, 32));
        MCK(mmi_lm_load_adapter(lm, 1, 2.0f, ad.data(), (int32_t)ad.size(), nullptr));
        mmi_sampling sp; memset(&sp, 0, sizeof(sp));
        sp.use_sampling = 0; sp.temp = 0.8f; sp.temp_text = 0.7f; sp.top_k = 250; sp.top_k_text = 25; sp.seed = 0;
        const int NT = dep_q + 1;
        const int64_t* eforced = (const int64_t*)expect("lm_forced");
        const int64_t* eout = (const int64_t*)expect("lm_out");
        const float* etl = (const float*)expect("lm_text_logits");
        int64_t *duc, *dforced, *dout; float *dtl, *dal;
        HCK(hipMalloc((void**)&duc, (size_t)B * n_user * 8)); HCK(hipMalloc((void**)&dforced, (size_t)B * NT * 8));
        HCK(hipMalloc((void**)&dout, (size_t)B * NT * 8));
        HCK(hipMalloc((void**)&dtl, (size_t)B * text_card * 4)); HCK(hipMalloc((void**)&dal, (size_t)B * dep_q * card * 4));
        std::vector<std::vector<float>> tls[2];
        long tok_diffs = 0; double worst_max = 0;
        int refused = 0;
        for (int pass = 0; pass < 2; ++pass) {            // pass 0: every row at -1; pass 1: row 0 on slot 1
            MCK(mmi_lm_streaming_start(lm, B, &sp, nullptr));
            if (pass) {
                MCK(mmi_lm_set_row_adapter(lm, 0, 1, nullptr));
                refused += mmi_lm_unload_adapter(lm, 1, nullptr) == MMI_ERR_STATE;
                refused += mmi_lm_load_adapter(lm, 1, 2.0f, ad.data(), (int32_t)ad.size(), nullptr) == MMI_ERR_STATE;
                refused += mmi_lm_row_adapter(lm, 0) == 1 && mmi_lm_row_adapter(lm, B - 1) == (B > 1 ? -1 : 1);
            }
            for (int s = 0; s < ST; ++s) {
                std::vector<int64_t> uc((size_t)B * n_user);
                for (size_t i = 0; i < uc.size(); ++i) uc[i] = (int64_t)((u_of(9000u + s, (uint32_t)i) + 1.0f) * 32768.0f) % card;
                HCK(hipMemcpy(duc, uc.data(), uc.size() * 8, hipMemcpyHostToDevice));
                HCK(hipMemcpy(dforced, eforced + (size_t)s * B * NT, (size_t)B * NT * 8, hipMemcpyHostToDevice));
                MCK(mmi_lm_force_next_tokens(lm, dforced, nullptr));
                int32_t valid = 0;
                MCK(mmi_lm_step(lm, duc, n_user, dout, dtl, dal, nullptr, B, &valid, nullptr));
                HCK(hipDeviceSynchronize());
                std::vector<int64_t> o((size_t)B * NT); std::vector<float> tl((size_t)B * text_card);
                HCK(hipMemcpy(o.data(), dout, o.size() * 8, hipMemcpyDeviceToHost));
                HCK(hipMemcpy(tl.data(), dtl, tl.size() * 4, hipMemcpyDeviceToHost));
                if (!pass) {
                    for (size_t i = 0; i < o.size(); ++i) tok_diffs += o[i] != eout[(size_t)s * B * NT + i];
                    for (int b = 0; b < B; ++b) {
                        double mx = 1e-6, dmax = 0;
                        for (int i = 0; i < text_card; ++i) {
                            const float r = etl[((size_t)s * B + b) * text_card + i];
                            mx = fmax(mx, fabs(r)); dmax = fmax(dmax, fabs(tl[(size_t)b * text_card + i] - r));
                        }
                        worst_max = fmax(worst_max, dmax / mx);
                    }
                }
                tls[pass].push_back(tl);
            }
            if (pass) { MCK(mmi_lm_set_row_adapter(lm, 0, -1, nullptr)); MCK(mmi_lm_unload_adapter(lm, 1, nullptr)); }
            MCK(mmi_lm_streaming_stop(lm));
        }
        long others_changed = 0, row0_changed = 0;
        for (int s = 0; s < ST; ++s) {
            row0_changed += memcmp(tls[0][s].data(), tls[1][s].data(), (size_t)text_card * 4) != 0;
            if (B > 1) others_changed += memcmp(tls[0][s].data() + text_card, tls[1][s].data() + text_card, (size_t)(B - 1) * text_card * 4) != 0;
        }
        printf("lm with adapters: rows at -1: %ld of %d token-ring outputs differ from the oracle (must be 0), text logits worst max %.4f (<= 0.05); "
               "row 0 on slot 1: its text logits changed in %ld of %d steps (must be all), the other rows' in %ld (must be 0); %d of 3 live-slot checks held\n",
               tok_diffs, ST * B * NT, worst_max, row0_changed, ST, others_changed, refused);
        failures += tok_diffs != 0 || !(worst_max <= 0.05) || row0_changed != ST || others_changed != 0 || refused != 3;
        MCK(mmi_lm_enable_adapters(lm, 0, 0));
        mmi_lm_destroy(lm);
        hipFree(duc); hipFree(dforced); hipFree(dout); hipFree(dtl); hipFree(dal);
        for (void* p : bufs) hipFree(p);
    }
    if (nucleus) {
        // Free-running (nothing forced): a sampling stream with top_p = top_p_text = 1e-6 on the nucleus samplers must give the greedy
        // stream's tokens - the nucleus is then the argmax alone, at every site - and the refusals of the entry points must hold.
        mmi_lm* lm = nullptr;
        MCK(mmi_lm_create(&lc, ld.data(), (int32_t)ld.size(), B, &lm));
        const int NT = dep_q + 1;
        int64_t *duc, *dout; float* dnoise;
        HCK(hipMalloc((void**)&duc, (size_t)B * n_user * 8)); HCK(hipMalloc((void**)&dout, (size_t)B * NT * 8));
        HCK(hipMalloc((void**)&dnoise, (size_t)B * NT * 250 * 4));
        {
            std::vector<float> ones((size_t)B * NT * 250, 1.0f);
            HCK(hipMemcpy(dnoise, ones.data(), ones.size() * 4, hipMemcpyHostToDevice));
        }
        int held = 0, checks = 0;
        auto holds = [&](int rc, int want) { ++checks; held += rc == want; if (rc != want) printf("  refusal check %d: status %d, expected %d\n", checks, rc, want); };
        float a = -1.f, t = -1.f;
        holds(mmi_lm_set_top_p(lm, 0.5f, 0.5f), MMI_ERR_STATE);                 // not enabled
        MCK(mmi_lm_enable_nucleus(lm, 1));
        holds(mmi_lm_set_top_p(lm, 1.5f, 0.f), MMI_ERR_INVALID);
        holds(mmi_lm_set_top_p(lm, 0.f, -0.5f), MMI_ERR_INVALID);
        holds(mmi_lm_set_top_p(lm, NAN, 0.f), MMI_ERR_INVALID);
        MCK(mmi_lm_top_p(lm, &a, &t));
        holds(a == 0.f && t == 0.f ? 0 : 1, 0);                                // the refused calls changed nothing
        holds(mmi_lm_set_row_top_p(lm, 0, 0.5f, 0.5f, nullptr), MMI_ERR_STATE); // not streaming
        std::vector<std::vector<int64_t>> toks[3];
        for (int pass = 0; pass < 3; ++pass) {            // 0: greedy; 1: sampling, top_p = 1e-6; 2: sampling, top-k (the control)
            mmi_sampling sp; memset(&sp, 0, sizeof(sp));
            sp.use_sampling = pass != 0; sp.temp = 0.8f; sp.temp_text = 0.7f; sp.top_k = 250; sp.top_k_text = 25; sp.seed = 5;
            MCK(mmi_lm_set_top_p(lm, pass == 1 ? 1e-6f : 0.f, pass == 1 ? 1e-6f : 0.f));
            MCK(mmi_lm_streaming_start(lm, B, &sp, nullptr));
            if (pass == 1) {
                holds(mmi_lm_enable_nucleus(lm, 0), MMI_ERR_STATE);             // while streaming
                holds(mmi_lm_set_top_p(lm, 0.f, 0.f), MMI_ERR_STATE);
                holds(mmi_lm_set_row_top_p(lm, B, 0.5f, 0.5f, nullptr), MMI_ERR_INVALID);
                holds(mmi_lm_set_row_top_p(lm, 0, 2.f, 0.5f, nullptr), MMI_ERR_INVALID);
            }
            for (int s = 0; s < ST; ++s) {
                std::vector<int64_t> uc((size_t)B * n_user);
                for (size_t i = 0; i < uc.size(); ++i) uc[i] = (int64_t)((u_of(9000u + s, (uint32_t)i) + 1.0f) * 32768.0f) % card;
                HCK(hipMemcpy(duc, uc.data(), uc.size() * 8, hipMemcpyHostToDevice));
                int32_t valid = 0;
                if (pass == 1 && s == 0) holds(mmi_lm_step(lm, duc, n_user, dout, nullptr, nullptr, dnoise, B, &valid, nullptr), MMI_ERR_UNSUPPORTED);
                if (pass == 2 && s == 1) {                // a session's own value refuses the noise too; cleared, the noise is accepted
                    MCK(mmi_lm_set_row_top_p(lm, B - 1, 0.f, 0.9f, nullptr));
                    holds(mmi_lm_step(lm, duc, n_user, dout, nullptr, nullptr, dnoise, B, &valid, nullptr), MMI_ERR_UNSUPPORTED);
                    MCK(mmi_lm_clear_row_top_p(lm, B - 1, nullptr));
                }
                MCK(mmi_lm_step(lm, duc, n_user, dout, nullptr, nullptr, nullptr, B, &valid, nullptr));
                HCK(hipDeviceSynchronize());
                std::vector<int64_t> o((size_t)B * NT);
                HCK(hipMemcpy(o.data(), dout, o.size() * 8, hipMemcpyDeviceToHost));
                toks[pass].push_back(o);
            }
            MCK(mmi_lm_streaming_stop(lm));
        }
        MCK(mmi_lm_set_top_p(lm, 0.f, 0.f));
        MCK(mmi_lm_enable_nucleus(lm, 0));
        mmi_sampling sp; memset(&sp, 0, sizeof(sp));
        sp.use_sampling = 1; sp.temp = 0.8f; sp.temp_text = 0.7f; sp.top_k = 250; sp.top_k_text = 25; sp.seed = 5;
        MCK(mmi_lm_streaming_start(lm, B, &sp, nullptr));
        holds(mmi_lm_set_row_top_p(lm, 0, 0.5f, 0.5f, nullptr), MMI_ERR_STATE);   // a stream without the nucleus samplers
        holds(mmi_lm_clear_row_top_p(lm, 0, nullptr), MMI_ERR_STATE);
        MCK(mmi_lm_streaming_stop(lm));
        long differ = 0, control = 0, produced = 0;
        for (int s = 0; s < ST; ++s)
            for (size_t i = 0; i < toks[0][s].size(); ++i) {
                differ += toks[0][s][i] != toks[1][s][i];
                control += toks[0][s][i] != toks[2][s][i];
                produced += toks[0][s][i] >= 0;
            }
        printf("lm with the nucleus samplers: top_p = 1e-6 differs from the greedy stream in %ld of %ld tokens (must be 0; the top-k stream "
               "differs in %ld: must be > 0); %d of %d refusal checks held\n", differ, produced, control, held, checks);
        failures += differ != 0 || control == 0 || produced == 0 || held != checks;
        mmi_lm_destroy(lm);
        hipFree(duc); hipFree(dout); hipFree(dnoise);
    }
    if (prefill) {
        // R sessions (session r replays the fixture's session r % B) take the first `cut` recorded frames by prefill under a row budget
        // `rows`, then the frames cut .. ST - 1 by forced steps: ring outputs (they still come out of the delay ring the prefill left)
        // and logits against the oracle's record
        const int NT = dep_q + 1, cut = ST / 2;
        const int64_t* eforced = (const int64_t*)expect("lm_forced");
        const int64_t* eout = (const int64_t*)expect("lm_out");
        const float* etl = (const float*)expect("lm_text_logits");
        const float* eal = (const float*)expect("lm_audio_logits");
        mmi_sampling sp; memset(&sp, 0, sizeof(sp));
        sp.use_sampling = 0; sp.temp = 0.8f; sp.temp_text = 0.7f; sp.top_k = 250; sp.top_k_text = 25; sp.seed = 0;
        int held = 0, checks = 0;
        auto holds = [&](int rc, int want) { ++checks; held += rc == want; if (rc != want) printf("  refusal check %d: status %d, expected %d\n", checks, rc, want); };
        struct Run { int R, rows; bool many; };
        for (const Run run : {Run{B, 2 * B, false}, Run{B, B, false}, Run{66, 128, true}}) {
            const int R = run.R;
            mmi_lm* lm = nullptr;
            if (run.many) MCK(mmi_lm_create_rows(&lc, nullptr, ld.data(), (int32_t)ld.size(), 128, &lm));
            else MCK(mmi_lm_create(&lc, ld.data(), (int32_t)ld.size(), B, &lm));
            int64_t *duc, *dforced, *dout, *dpu, *dpt, *dlast; float *dtl, *dal;
            HCK(hipMalloc((void**)&duc, (size_t)R * n_user * 8)); HCK(hipMalloc((void**)&dforced, (size_t)R * NT * 8));
            HCK(hipMalloc((void**)&dout, (size_t)R * NT * 8)); HCK(hipMalloc((void**)&dlast, (size_t)R * NT * 8));
            HCK(hipMalloc((void**)&dpu, (size_t)R * n_user * cut * 8)); HCK(hipMalloc((void**)&dpt, (size_t)R * NT * cut * 8));
            HCK(hipMalloc((void**)&dtl, (size_t)R * text_card * 4)); HCK(hipMalloc((void**)&dal, (size_t)R * dep_q * card * 4));
            std::vector<int32_t> sess(R);
            for (int r = 0; r < R; ++r) sess[r] = r;
            if (!run.many && run.rows == 2 * B) {
                holds(mmi_lm_prefill_rows(lm), 0);
                holds(mmi_lm_enable_prefill(lm, 129), MMI_ERR_UNSUPPORTED);
                holds(mmi_lm_enable_prefill(lm, 33), MMI_ERR_UNSUPPORTED);             // a handle of the 16-row tile
                MCK(mmi_lm_streaming_start(lm, R, &sp, nullptr));
                holds(mmi_lm_prefill(lm, sess.data(), R, dpu, dpt, cut, nullptr), MMI_ERR_STATE);      // not enabled
                holds(mmi_lm_enable_prefill(lm, 4), MMI_ERR_STATE);                    // while streaming
                MCK(mmi_lm_streaming_stop(lm));
            }
            MCK(mmi_lm_enable_prefill(lm, run.rows));
            MCK(mmi_lm_streaming_start(lm, R, &sp, nullptr));
            const int64_t bytes_with = mmi_lm_state_bytes(lm);
            std::vector<int64_t> pu((size_t)R * n_user * cut), pt((size_t)R * NT * cut);
            for (int f = 0; f < cut; ++f) {
                std::vector<int64_t> uc1((size_t)B * n_user);
                for (size_t i = 0; i < uc1.size(); ++i) uc1[i] = (int64_t)((u_of(9000u + f, (uint32_t)i) + 1.0f) * 32768.0f) % card;
                for (int r = 0; r < R; ++r) {
                    for (int c = 0; c < n_user; ++c) pu[((size_t)r * n_user + c) * cut + f] = uc1[(size_t)(r % B) * n_user + c];
                    for (int c = 0; c < NT; ++c) pt[((size_t)r * NT + c) * cut + f] = eforced[((size_t)f * B + r % B) * NT + c];
                }
            }
            HCK(hipMemcpy(dpu, pu.data(), pu.size() * 8, hipMemcpyHostToDevice));
            HCK(hipMemcpy(dpt, pt.data(), pt.size() * 8, hipMemcpyHostToDevice));
            if (!run.many && run.rows == 2 * B) {
                std::vector<int32_t> twice(R, 0);
                holds(R > 1 ? mmi_lm_prefill(lm, twice.data(), R, dpu, dpt, cut, nullptr) : MMI_ERR_INVALID, MMI_ERR_INVALID);
                holds(mmi_lm_prefill(lm, sess.data(), R, dpu, dpt, 0, nullptr), MMI_ERR_INVALID);
                holds(mmi_lm_prefill(lm, sess.data(), run.rows + 1, dpu, dpt, cut, nullptr), MMI_ERR_INVALID);
            }
            MCK(mmi_lm_prefill(lm, sess.data(), R, dpu, dpt, cut, nullptr));
            MCK(mmi_lm_last_tokens(lm, dlast, nullptr));
            HCK(hipDeviceSynchronize());
            std::vector<int64_t> last((size_t)R * NT);
            HCK(hipMemcpy(last.data(), dlast, last.size() * 8, hipMemcpyDeviceToHost));
            long last_diffs = 0, tok_diffs = 0; double worst_max = 0, worst_mean = 0;
            for (int r = 0; r < R; ++r)
                for (int c = 0; c < NT; ++c) last_diffs += last[(size_t)r * NT + c] != eforced[((size_t)(cut - 1) * B + r % B) * NT + c];
            auto site = [&](const float* a, const float* r, int n) {
                double mx = 1e-6, dmax = 0, dsum = 0;
                for (int i = 0; i < n; ++i) { mx = fmax(mx, fabs(r[i])); const double d = fabs(a[i] - r[i]); dmax = fmax(dmax, d); dsum += d; }
                worst_max = fmax(worst_max, dmax / mx); worst_mean = fmax(worst_mean, dsum / n / mx);
            };
            for (int s = cut; s < ST; ++s) {
                std::vector<int64_t> uc1((size_t)B * n_user), uc((size_t)R * n_user), fo((size_t)R * NT);
                for (size_t i = 0; i < uc1.size(); ++i) uc1[i] = (int64_t)((u_of(9000u + s, (uint32_t)i) + 1.0f) * 32768.0f) % card;
                for (int r = 0; r < R; ++r) {
                    memcpy(uc.data() + (size_t)r * n_user, uc1.data() + (size_t)(r % B) * n_user, (size_t)n_user * 8);
                    memcpy(fo.data() + (size_t)r * NT, eforced + ((size_t)s * B + r % B) * NT, (size_t)NT * 8);
                }
                HCK(hipMemcpy(duc, uc.data(), uc.size() * 8, hipMemcpyHostToDevice));
                HCK(hipMemcpy(dforced, fo.data(), fo.size() * 8, hipMemcpyHostToDevice));
                MCK(mmi_lm_force_next_tokens(lm, dforced, nullptr));
                int32_t valid = 0;
                MCK(mmi_lm_step(lm, duc, n_user, dout, dtl, dal, nullptr, R, &valid, nullptr));
                HCK(hipDeviceSynchronize());
                std::vector<int64_t> o((size_t)R * NT); std::vector<float> tl((size_t)R * text_card), al((size_t)R * dep_q * card);
                HCK(hipMemcpy(o.data(), dout, o.size() * 8, hipMemcpyDeviceToHost));
                HCK(hipMemcpy(tl.data(), dtl, tl.size() * 4, hipMemcpyDeviceToHost));
                HCK(hipMemcpy(al.data(), dal, al.size() * 4, hipMemcpyDeviceToHost));
                for (int r = 0; r < R; ++r) {
                    const int b = r % B;
                    for (int i = 0; i < NT; ++i) tok_diffs += o[(size_t)r * NT + i] != eout[((size_t)s * B + b) * NT + i];
                    site(tl.data() + (size_t)r * text_card, etl + ((size_t)s * B + b) * text_card, text_card);
                    for (int k = 0; k < dep_q; ++k) site(al.data() + ((size_t)r * dep_q + k) * card, eal + (((size_t)s * B + b) * dep_q + k) * card, card);
                }
            }
            MCK(mmi_lm_streaming_stop(lm));
            MCK(mmi_lm_enable_prefill(lm, 0));
            MCK(mmi_lm_streaming_start(lm, R, &sp, nullptr));
            const int64_t bytes_without = mmi_lm_state_bytes(lm);
            MCK(mmi_lm_streaming_stop(lm));
            printf("lm prefill, %d sessions, %d rows per pass (%lld k_gemm_rows launches): %d frames prefilled; last_tokens differ in %ld entries (must be 0); "
                   "%ld of %d token-ring outputs of the next %d steps differ from the oracle (must be 0); logits worst max %.4f (<= 0.05), worst mean "
                   "%.4f (<= 0.012); state bytes %lld with, %lld without (must be equal)\n", R, run.rows, (long long)mmi_lm_stat(lm, 4), cut, last_diffs,
                   tok_diffs, (ST - cut) * R * NT, ST - cut, worst_max, worst_mean, (long long)bytes_with, (long long)bytes_without);
            failures += last_diffs != 0 || tok_diffs != 0 || !(worst_max <= 0.05) || !(worst_mean <= 0.012) || bytes_with != bytes_without ||
                        (run.many && mmi_lm_stat(lm, 4) <= 0) || cut < 1;
            mmi_lm_destroy(lm);
            hipFree(duc); hipFree(dforced); hipFree(dout); hipFree(dlast); hipFree(dpu); hipFree(dpt); hipFree(dtl); hipFree(dal);
        }
        printf("lm prefill: %d of %d refusal checks held\n", held, checks);
        failures += held != checks;
    }
    if (score) {
        // The fixture's sessions take the first `cut` recorded frames through mmi_lm_score (commit = 1) under a row budget `rows`: its logits
        // against the step logits the oracle recorded for those frames, logp against the double-precision log-softmax of the returned
        // logits, argmax against theirs; then the frames cut .. ST - 1 by forced steps against the record, as after a prefill
        const int NT = dep_q + 1, cut = ST / 2;
        const int64_t* eforced = (const int64_t*)expect("lm_forced");
        const int64_t* eout = (const int64_t*)expect("lm_out");
        const float* etl = (const float*)expect("lm_text_logits");
        const float* eal = (const float*)expect("lm_audio_logits");
        mmi_sampling sp; memset(&sp, 0, sizeof(sp));
        sp.use_sampling = 0; sp.temp = 0.8f; sp.temp_text = 0.7f; sp.top_k = 250; sp.top_k_text = 25; sp.seed = 0;
        int held = 0, checks = 0;
        auto holds = [&](int rc, int want) { ++checks; held += rc == want; if (rc != want) printf("  refusal check %d: status %d, expected %d\n", checks, rc, want); };
        for (int run = 0; run < 2; ++run) {
            const int R = B, rows = run ? B : (B * cut <= 32 ? B * cut : 2 * B);      // all scored frames in one pass; passes of one frame
            mmi_lm* lm = nullptr;
            MCK(mmi_lm_create(&lc, ld.data(), (int32_t)ld.size(), B, &lm));
            int64_t *duc, *dforced, *dout, *dpu, *dpt; float *dtl, *dal, *dlogp, *dstl, *dsal; int32_t* dam;
            HCK(hipMalloc((void**)&duc, (size_t)R * n_user * 8)); HCK(hipMalloc((void**)&dforced, (size_t)R * NT * 8));
            HCK(hipMalloc((void**)&dout, (size_t)R * NT * 8));
            HCK(hipMalloc((void**)&dpu, (size_t)R * n_user * cut * 8)); HCK(hipMalloc((void**)&dpt, (size_t)R * NT * cut * 8));
            HCK(hipMalloc((void**)&dtl, (size_t)R * text_card * 4)); HCK(hipMalloc((void**)&dal, (size_t)R * dep_q * card * 4));
            HCK(hipMalloc((void**)&dlogp, (size_t)R * cut * NT * 4)); HCK(hipMalloc((void**)&dam, (size_t)R * cut * NT * 4));
            HCK(hipMalloc((void**)&dstl, (size_t)R * cut * text_card * 4)); HCK(hipMalloc((void**)&dsal, (size_t)R * cut * dep_q * card * 4));
            std::vector<int32_t> sess(R);
            for (int r = 0; r < R; ++r) sess[r] = r;
            mmi_score_out so; so.logp = dlogp; so.argmax = dam; so.text_logits = dstl; so.audio_logits = dsal;
            const bool first = run == 0;
            if (first) {
                holds(mmi_lm_score_enabled(lm), 0);
                holds(mmi_lm_enable_score(lm, 1), MMI_ERR_STATE);                      // prefill is not enabled
                MCK(mmi_lm_enable_prefill(lm, rows));
                MCK(mmi_lm_streaming_start(lm, R, &sp, nullptr));
                holds(mmi_lm_score(lm, sess.data(), R, dpu, dpt, cut, 1, &so, nullptr), MMI_ERR_STATE);     // scoring is not enabled
                holds(mmi_lm_enable_score(lm, 1), MMI_ERR_STATE);                      // while streaming
                MCK(mmi_lm_streaming_stop(lm));
            }
            MCK(mmi_lm_enable_prefill(lm, rows));
            MCK(mmi_lm_enable_score(lm, 1));
            MCK(mmi_lm_streaming_start(lm, R, &sp, nullptr));
            const int64_t bytes_with = mmi_lm_state_bytes(lm);
            std::vector<int64_t> pu((size_t)R * n_user * cut), pt((size_t)R * NT * cut);
            for (int f = 0; f < cut; ++f) {
                std::vector<int64_t> uc1((size_t)B * n_user);
                for (size_t i = 0; i < uc1.size(); ++i) uc1[i] = (int64_t)((u_of(9000u + f, (uint32_t)i) + 1.0f) * 32768.0f) % card;
                for (int r = 0; r < R; ++r) {
                    for (int c = 0; c < n_user; ++c) pu[((size_t)r * n_user + c) * cut + f] = uc1[(size_t)r * n_user + c];
                    for (int c = 0; c < NT; ++c) pt[((size_t)r * NT + c) * cut + f] = eforced[((size_t)f * B + r) * NT + c];
                }
            }
            HCK(hipMemcpy(dpu, pu.data(), pu.size() * 8, hipMemcpyHostToDevice));
            HCK(hipMemcpy(dpt, pt.data(), pt.size() * 8, hipMemcpyHostToDevice));
            if (first) {
                mmi_score_out bad = so; bad.logp = nullptr;
                holds(mmi_lm_score(lm, sess.data(), R, dpu, dpt, cut, 1, &bad, nullptr), MMI_ERR_INVALID);          // a null logp
                holds(mmi_lm_score(lm, sess.data(), R, dpu, dpt, cut, 1, nullptr, nullptr), MMI_ERR_INVALID);
                holds(mmi_lm_score(lm, sess.data(), R, dpu, dpt, 0, 1, &so, nullptr), MMI_ERR_INVALID);
                holds(mmi_lm_score(lm, sess.data(), R, dpu, dpt, rows / R + 1, 0, &so, nullptr), MMI_ERR_INVALID);   // commit = 0 beyond one pass
                std::vector<int32_t> twice(R, 0);
                holds(R > 1 ? mmi_lm_score(lm, twice.data(), R, dpu, dpt, cut, 1, &so, nullptr) : MMI_ERR_INVALID, MMI_ERR_INVALID);
            }
            MCK(mmi_lm_score(lm, sess.data(), R, dpu, dpt, cut, 1, &so, nullptr));
            HCK(hipDeviceSynchronize());
            std::vector<float> lp((size_t)R * cut * NT), stl((size_t)R * cut * text_card), sal((size_t)R * cut * dep_q * card);
            std::vector<int32_t> am((size_t)R * cut * NT);
            HCK(hipMemcpy(lp.data(), dlogp, lp.size() * 4, hipMemcpyDeviceToHost));
            HCK(hipMemcpy(am.data(), dam, am.size() * 4, hipMemcpyDeviceToHost));
            HCK(hipMemcpy(stl.data(), dstl, stl.size() * 4, hipMemcpyDeviceToHost));
            if (dep_q) HCK(hipMemcpy(sal.data(), dsal, sal.size() * 4, hipMemcpyDeviceToHost));
            long tok_diffs = 0, am_diffs = 0; double worst_max = 0, worst_mean = 0, worst_logp = 0;
            auto site = [&](const float* a, const float* r, int n) {
                double mx = 1e-6, dmax = 0, dsum = 0;
                for (int i = 0; i < n; ++i) { mx = fmax(mx, fabs(r[i])); const double d = fabs(a[i] - r[i]); dmax = fmax(dmax, d); dsum += d; }
                worst_max = fmax(worst_max, dmax / mx); worst_mean = fmax(worst_mean, dsum / n / mx);
            };
            // logp and argmax of one site against the double-precision values from the returned row
            auto own = [&](const float* row, int n, int64_t tok, float got_lp, int got_am) {
                double mx = -INFINITY, sum = 0; int best = 0;
                for (int i = 0; i < n; ++i) if ((double)row[i] > mx) { mx = row[i]; best = i; }
                for (int i = 0; i < n; ++i) sum += exp((double)row[i] - mx);
                am_diffs += best != got_am;
                if (tok >= 0 && tok < n) worst_logp = fmax(worst_logp, fabs((double)got_lp - (((double)row[tok] - mx) - log(sum))));
                else worst_logp = fmax(worst_logp, got_lp == -INFINITY ? 0.0 : 1.0);
            };
            for (int r = 0; r < R; ++r)
                for (int f = 0; f < cut; ++f) {
                    const size_t rf = (size_t)r * cut + f;
                    site(stl.data() + rf * text_card, etl + ((size_t)f * B + r) * text_card, text_card);
                    own(stl.data() + rf * text_card, text_card, eforced[((size_t)f * B + r) * NT], lp[rf * NT], am[rf * NT]);
                    for (int k = 0; k < dep_q; ++k) {
                        site(sal.data() + (rf * dep_q + k) * card, eal + (((size_t)f * B + r) * dep_q + k) * card, card);
                        own(sal.data() + (rf * dep_q + k) * card, card, eforced[((size_t)f * B + r) * NT + 1 + k], lp[rf * NT + 1 + k], am[rf * NT + 1 + k]);
                    }
                }
            for (int s = cut; s < ST; ++s) {
                std::vector<int64_t> uc((size_t)R * n_user);
                for (size_t i = 0; i < uc.size(); ++i) uc[i] = (int64_t)((u_of(9000u + s, (uint32_t)i) + 1.0f) * 32768.0f) % card;
                HCK(hipMemcpy(duc, uc.data(), uc.size() * 8, hipMemcpyHostToDevice));
                HCK(hipMemcpy(dforced, eforced + (size_t)s * B * NT, (size_t)B * NT * 8, hipMemcpyHostToDevice));
                MCK(mmi_lm_force_next_tokens(lm, dforced, nullptr));
                int32_t valid = 0;
                MCK(mmi_lm_step(lm, duc, n_user, dout, dtl, dal, nullptr, R, &valid, nullptr));
                HCK(hipDeviceSynchronize());
                std::vector<int64_t> o((size_t)R * NT); std::vector<float> tl((size_t)R * text_card), al((size_t)R * dep_q * card);
                HCK(hipMemcpy(o.data(), dout, o.size() * 8, hipMemcpyDeviceToHost));
                HCK(hipMemcpy(tl.data(), dtl, tl.size() * 4, hipMemcpyDeviceToHost));
                if (dep_q) HCK(hipMemcpy(al.data(), dal, al.size() * 4, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < o.size(); ++i) tok_diffs += o[i] != eout[(size_t)s * B * NT + i];
                for (int b = 0; b < B; ++b) {
                    site(tl.data() + (size_t)b * text_card, etl + ((size_t)s * B + b) * text_card, text_card);
                    for (int k = 0; k < dep_q; ++k) site(al.data() + ((size_t)b * dep_q + k) * card, eal + (((size_t)s * B + b) * dep_q + k) * card, card);
                }
            }
            MCK(mmi_lm_streaming_stop(lm));
            MCK(mmi_lm_enable_score(lm, 0));
            MCK(mmi_lm_streaming_start(lm, R, &sp, nullptr));
            const int64_t bytes_without = mmi_lm_state_bytes(lm);
            MCK(mmi_lm_streaming_stop(lm));
            printf("lm score, %d sessions, %d rows per pass: %d frames scored; logits of the scored frames and of the next %d steps worst max %.4f "
                   "(<= 0.05), worst mean %.4f (<= 0.012) of max|logit|; logp worst %.3g from its own logits (<= 2^-13); argmax differs in %ld sites "
                   "(must be 0); %ld of %d token-ring outputs of the next steps differ from the oracle (must be 0); state bytes %lld with, %lld without "
                   "(must be equal)\n", R, rows, cut, ST - cut, worst_max, worst_mean, worst_logp, am_diffs, tok_diffs, (ST - cut) * R * NT,
                   (long long)bytes_with, (long long)bytes_without);
            failures += tok_diffs != 0 || am_diffs != 0 || !(worst_max <= 0.05) || !(worst_mean <= 0.012) || !(worst_logp <= 1.0 / 8192) ||
                        bytes_with != bytes_without || cut < 1;
            mmi_lm_destroy(lm);
            hipFree(duc); hipFree(dforced); hipFree(dout); hipFree(dpu); hipFree(dpt); hipFree(dtl); hipFree(dal);
            hipFree(dlogp); hipFree(dam); hipFree(dstl); hipFree(dsal);
        }
        printf("lm score: %d of %d refusal checks held\n", held, checks);
        failures += held != checks;
    }
    printf(failures ? "SELFTEST FAILED\n" : "SELFTEST PASSED\n");
    return failures ? 1 : 0;
}
