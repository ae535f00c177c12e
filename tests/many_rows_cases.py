"""Cases for an LM handle of 65..128 model rows (`LMModel(max_rows=)`, mmi_lm_create_rows, k_gemm_rows), shared by the simulator
tests (tests/test_many_rows_sim.py) and the GPU tests (tests/test_b_many_rows_gpu.py).

The checkers of the other case modules build their engines with `LMModel(..., max_batch=rows)`.  `rows_shim()` lets them run
above 64 rows unchanged: inside it such a request is made through `max_rows` (what a caller has to write), nothing else moves."""
from __future__ import annotations

import contextlib
import os
from dataclasses import replace

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config, tiny_stt_config
from moshi_amd.lm import LMGen, LMModel, SessionSampling
from oracle.lm_oracle import bf16r, silu
from tests import lm_cases as lc
from tests.lm_cases import _bf16_bits, _dyadic_rows, cached_lm_state_dict


@contextlib.contextmanager
def rows_shim():
    init = LMModel.__init__

    def patched(self, *a, max_batch=32, **kw):
        if max_batch > 64 and kw.get("max_rows") is None:
            return init(self, *a, max_rows=max_batch, **kw)
        return init(self, *a, max_batch=max_batch, **kw)
    LMModel.__init__ = patched
    try:
        yield
    finally:
        LMModel.__init__ = init


@contextlib.contextmanager
def env(**kv):
    """MMI_* variables are read once, when a handle is created: set them around the LMModel(...) call."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rows_launches(gen_or_lm):
    lm = getattr(gen_or_lm, "lm_model", gen_or_lm)
    return int(lm._lib.mmi_lm_stat(lm._handle, 4))


# ---- 1. every linear family on exact sums ------------------------------------------------------------------------------------------------
# The rule of lm_cases.int8_linears_bit_exact: a plain linear's bf16 output IDENTICAL to the reference, a gated one (SiLU goes
# through the device's exp) >= 99.9 % identical and everything within one bf16 step (2^-7 relative).  For bf16 linears the reference
# is the float64 sum of the bf16 operands, and the rule can be asked of an fp32 accumulator only where that sum is exact in fp32 in
# ANY order: weights on the grid k * 2^-10, |k| <= 255 (bf16 values), rows of +-2^-2..2^1 (_dyadic_rows): every product is a multiple
# of 2^-12, every partial sum of up to 352 of them stays below 2^24 such units.  What is left is indexing, the K partition, the
# reduction and the epilogue - what a new GEMM kernel can get wrong.
LINEAR_ROWS = (65, 96, 97, 128)


def grid_state_dict(cfg, seed):
    sd = cached_lm_state_dict(cfg, seed)
    for k, v in sd.items():
        if v.ndim == 2 and k.endswith(".weight") and "emb" not in k:
            w = v.float()
            sd[k] = (torch.round(w / w.abs().max() * 255.0).clamp(-255, 255) / 1024.0).to(torch.bfloat16)
    return sd


def linear_sites(cfg):
    k_last = cfg.dep_q - 1
    return [
        ("transformer.layers.0.self_attn.in_projs.0.weight", ["plain"]),                 # K = 128: 2 k-steps per wave
        ("transformer.layers.0.self_attn.out_projs.0.weight", ["plain", "splitk"]),
        ("transformer.layers.0.gating.linear_in.weight", ["plain"]),                     # gated, N = 352
        ("transformer.layers.1.gating.linear_out.weight", ["plain", "splitk"]),          # K = 352: 22 k-steps over 4 waves x 2
        ("text_linear.weight", ["plain"]),
        ("depformer_in.1.weight", ["plain"]),
        (f"depformer.layers.0.self_attn.in_projs.{k_last}.weight", ["plain"]),           # K = 64: one k-step per wave (remainder path)
        (f"depformer.layers.1.gating.{k_last}.linear_in.weight", ["plain"]),             # gated, N = 176: no multiple of 32
        ("depformer.layers.0.gating.2.linear_out.weight", ["plain", "splitk"]),          # K = 176: 11 k-steps, slices 3 / 3 / 3 / 2
        ("linears.3.weight", ["plain"]),                                                  # N = 72: the last n-tile holds 8 features
    ]


def check_linears_exact(device, lib, ntw=None, ksplit=None, seed=31):
    cfg = replace(tiny_lm_config(), card=72)
    sd = grid_state_dict(cfg, seed)
    knobs = {}
    if ntw:
        knobs["MMI_ROWS_NTW"] = ntw
    if ksplit:
        knobs["MMI_GEMM_KSPLIT"] = ksplit
    with env(**knobs):
        lm = LMModel(sd, cfg, device=device, max_rows=128, lib=lib)
    assert lm.max_batch == 128
    rng = np.random.default_rng(seed)
    checked = split = 0
    for key, paths in linear_sites(cfg):
        w = sd[key].float().numpy().astype(np.float64)
        gated = "linear_in" in key
        for path in paths:
            for B in LINEAR_ROWS:
                x = _dyadic_rows(rng, B, w.shape[1])
                try:
                    out = lm.debug_linear(key, torch.from_numpy(x), path=path)["out"].float().cpu().numpy()
                except NotImplementedError as e:
                    if path == "splitk" and "does not split" in str(e):      # tiny shapes are not split over K unless forced
                        continue
                    raise
                h = bf16r((x.astype(np.float64) @ w.T).astype(np.float32))     # the float64 sum is exact, and so is its fp32 copy
                if gated:
                    H = h.shape[1] // 2
                    ref = bf16r(bf16r(silu(h[:, :H])) * h[:, H:])
                else:
                    ref = h
                name = f"{key} [{path}] rows={B}"
                same = _bf16_bits(out) == _bf16_bits(ref)
                if gated:
                    ulp = np.abs(out - ref) <= np.maximum(np.abs(ref), 1e-30) * 2.0 ** -7
                    assert same.mean() >= 0.999 and ulp.all(), f"{name}: gated output {same.mean():.5f} identical, worst {np.abs(out - ref).max()}"
                else:
                    assert same.all(), f"{name}: {int((~same).sum())} of {same.size} bf16 outputs differ (first at {np.argwhere(~same)[0]})"
                checked += 1
                split += path == "splitk"
    if ksplit and ksplit > 1:
        assert split >= 2 * len(LINEAR_ROWS), f"MMI_GEMM_KSPLIT={ksplit}: only {split} split-K cases ran (MMI_EPI_PARTIAL not exercised)"
    return checked


# ---- 2. network against the oracle -------------------------------------------------------------------------------------------------------
def check_network_vs_oracle(device, lib, kind, B, kv="bf16"):
    """kv = "fp8": the e4m3 KV ring (the kv8 branch of the RoPE epilogue above two batch tiles), held to the oracle the way
    tests/test_lm_sim.py::test_fp8_kv_ring_matches_the_oracle does at <= 64 rows."""
    cfg = tiny_lm_config() if kind == "moshi" else tiny_stt_config()
    if kv != "bf16":
        cfg = replace(cfg, kv_cache_dtype=kv)
    stats = {}
    with rows_shim():
        lc.oracle_vs_engine(device, lib, cfg, seed=1300 + B, B=B, S=2, use_masks=True, stats=stats)
    kernels = {k for _, k in stats["launch_list"]}
    assert "k_gemm_rows" in kernels, kernels
    assert not kernels & {"k_gemm_xp", "k_gemm_xlds", "k_gemm_xp_norm", "k_gemm_xp_once", "k_dep_attn_out_proj"}, kernels
    assert stats["xlds_launches"] == 0


# ---- 3. a row does not depend on its tile ------------------------------------------------------------------------------------------------
TILE_SLOTS = (1, 33, 70, 127)


def check_rows_do_not_depend_on_their_tile(device, lib, steps=12):
    cfg = tiny_lm_config()
    B = 128
    lm = LMModel(cached_lm_state_dict(cfg, 21), cfg, device=device, max_rows=B, lib=lib)
    logits = []
    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=5, support_out_of_sync=True,
                on_text_logits_hook=lambda lg: logits.append(lg.view(torch.int16)[:, 0, 0].cpu().clone()))
    rng = np.random.default_rng(8)
    mine = SessionSampling(temp=0.7, temp_text=0.9, top_k=12, top_k_text=7, seed=4242)
    outs = []
    with gen.streaming(B):
        mask = [b in TILE_SLOTS for b in range(B)]
        gen.set_session_sampling([mine if m else SessionSampling() for m in mask], mask=mask)
        for s in range(steps):
            codes = rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))
            codes[list(TILE_SLOTS)] = codes[TILE_SLOTS[0]]                  # the same inputs for the sessions under test
            out = gen.step(torch.from_numpy(codes).to(device))
            outs.append(np.full((B, 1 + cfg.dep_q), -2, np.int64) if out is None else out[:, :, 0].cpu().numpy())
        assert rows_launches(gen) > 0
    a = TILE_SLOTS[0]
    for s in range(steps):
        for b in TILE_SLOTS[1:]:
            assert np.array_equal(outs[s][a], outs[s][b]), f"step {s}: tokens of slot {b} differ from slot {a}"
            assert torch.equal(logits[s][a], logits[s][b]), f"step {s}: text logits of slot {b} differ from slot {a} in bits"
    assert any((o[a] >= 0).all() for o in outs), "no step produced tokens: nothing shown"
    assert not np.array_equal(outs[-1][a], outs[-1][0]), "a session with other inputs gives the same tokens: nothing shown"


# ---- 4. guidance across the tile boundary ------------------------------------------------------------------------------------------------
def check_guided_sessions_vs_oracle(device, lib, sessions=40, steps=2):
    """40 guided sessions = 80 model rows: twin 40 + b sits in another batch tile than b.  Every session has its own guidance
    coefficient, sum condition and cross-attention source of its own length, and is held against a one-session oracle
    (row_condition_cases.check_sessions_vs_oracle, gates unchanged)."""
    from tests import row_condition_cases as rcc
    coefs = [(1.5, 2.0, 1.0, 3.0)[b % 4] for b in range(sessions)]
    lengths = [3 + (5 * b) % 15 for b in range(sessions)]
    with rows_shim():
        rcc.check_sessions_vs_oracle(device, lib, rcc.tiny_cross_config(), coefs, lengths, steps)
        lm = rcc.model(device, lib, rcc.tiny_cross_config(), 2 * sessions)
    assert lm.max_batch == 2 * sessions and rows_launches(lm) > 0


def check_tts_guided_sessions_vs_reference(device, lib, sessions=40):
    """The TTS-shaped model (tiny_tts_config: demuxed + low-rank embeddings, 20 micro-steps on a weight schedule, cross
    attention) with the script machine on, 40 guided sessions = 80 model rows (twin 40 + b in another batch tile than b).  The
    one-session reference is the reference's own teacher-forced run of tests/golden/lm_tts_machine.npz (three sessions, each
    with its condition, script and prefix; rows never mix): session b replays golden session b % 3 - so every golden session sits
    in slots on both sides of the 32-row boundary, and their twins on both sides of the 64-row boundary.  The stream starts with
    session 0's condition and another coefficient for everybody; every session then gets its own condition and cfg_coef through
    set_session_condition.  Held to tts_machine_cases.check_whole_step_against_reference's gates, unchanged."""
    from moshi_amd.config import tiny_tts_config
    from moshi_amd.lm import ConditionFuser, SessionCondition
    from moshi_amd.weights import random_lm_state_dict
    from tests import tts_machine_cases as tm
    g = tm.golden("lm_tts_machine.npz")
    S, GB = g["text_tok"].shape
    cfg = tiny_tts_config()
    dep_q = cfg.dep_q
    lm = LMModel(random_lm_state_dict(cfg, seed=int(g["seed"][0])), cfg, device=device, max_rows=2 * sessions, lib=lib,
                 fuser=ConditionFuser({"sum": ["s"], "cross": ["x"]}))
    t = lambda k: torch.from_numpy(g[k]).to(torch.bfloat16)
    cs, cx = t("sum"), t("cross")

    def cond_of(rows):
        return {"s": (cs[rows], torch.ones(len(rows), 1, dtype=torch.bool)), "x": (cx[rows], torch.ones(len(rows), cx.shape[1], dtype=torch.bool))}
    src = [b % GB for b in range(sessions)]
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=3.0, cfg_is_no_text=True,
                condition_tensors=cond_of([0] * sessions + [GB] * sessions), tts_machine=tm.lm_machine(g))
    gen.streaming_forever(sessions)
    try:
        for b, i in enumerate(src):
            gen.set_session_condition(b, SessionCondition(cfg_coef=2.0, condition_tensors=cond_of([i, GB + i])))
            gen.set_session_script(b, tm.lm_scripts(g)[i])
        for s_ in range(S):
            forced = np.concatenate([g["text_tok"][s_][:, None], g["audio_tok"][s_]], 1)[src]
            out, tl, al = gen.step_with_taps(tm.codes_for(gen, sessions), forced_tokens=torch.from_numpy(forced))
            out, tl, al = out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy()
            for b, i in enumerate(src):
                assert np.array_equal(out[b], g["tokens"][s_][i]), f"step {s_} session {b} (golden {i}): ring output differs"
                assert lc.logits_close(tl[b], g["text_logits"][s_, i]), f"step {s_} session {b}: text logits"
                for k in range(dep_q):
                    assert lc.logits_close(al[b, k], g["audio_logits"][s_, i, k], lc.GUIDED_WIDEN), f"step {s_} session {b} cb {k}: audio logits"
        for b, i in enumerate(src):
            st = gen.session_script_status(b)
            assert (-1 if st.end_step is None else st.end_step) == int(g["end_steps"][i]) and st.consumption_times == g[f"times{i}"].tolist(), b
        kernels = {k for _, k in gen.launch_list()}
        assert "k_gemm_rows" in kernels and "k_tts_machine" in kernels and rows_launches(gen) > 0, kernels
    finally:
        gen._stop_streaming()


# ---- 5. repeat streams -------------------------------------------------------------------------------------------------------------------
def check_repeat_streams(device, lib, B, repeats=2):
    with rows_shim():
        lc.reproducible_between_streams(device, lib, tiny_lm_config(), B, steps=3, repeats=repeats, seed=77 + B)


# ---- 6. snapshot -------------------------------------------------------------------------------------------------------------------------
def check_snapshot(device, lib, B=100):
    cfg = tiny_lm_config()
    lm = LMModel(cached_lm_state_dict(cfg, 21), cfg, device=device, max_rows=B, lib=lib)
    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=5, support_out_of_sync=True)
    rng = np.random.default_rng(12)
    codes = [torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device) for _ in range(6)]

    def run(cs):
        return [tuple(t.cpu().clone() for t in gen.step_with_taps(c)) for c in cs]
    with gen.streaming(B):
        run(codes[:3])
        snap = gen.get_streaming_state()
        first = run(codes[3:])
        run(codes[:1])                                      # wander off
        gen.set_streaming_state(snap)
        again = run(codes[3:])
        assert rows_launches(gen) > 0
    for s, (a, b) in enumerate(zip(first, again)):
        for name, x, y in zip(("tokens", "text logits", "audio logits"), a, b):
            assert torch.equal(x, y), f"step {s} after the snapshot: {name} differ"
    assert (first[-1][0] >= 0).all()


# ---- 7. the batcher ----------------------------------------------------------------------------------------------------------------------
def check_batcher(device, lib, slots=40):
    """SessionBatcher(slots=40, cfg_coef=1.5) on a max_rows=80 LM against the same schedule by hand (batcher_cases' checker); 36
    channels open at once, two of the slots above 32 are closed and taken again."""
    from moshi_amd.batcher import SessionBatcher
    from tests import batcher_cases as bc
    from moshi_amd.lm import ConditionFuser
    lcfg = tiny_lm_config()
    rng = np.random.default_rng(3)
    cond = torch.from_numpy(0.5 * rng.standard_normal((2 * slots, 1, lcfg.dim)).astype(np.float32)).to(torch.bfloat16)
    fuser = ConditionFuser({"sum": ["c"]})          # guidance needs a fuser (lm.py): one shared `sum` condition, as batcher_cases does
    with rows_shim():
        mimi_a, lm_a, mcfg, _ = bc.tiny_pair(device, lib, slots, lm_rows=2 * slots, fuser=fuser)
        mimi_b, lm_b, _, _ = bc.tiny_pair(device, lib, slots, lm_rows=2 * slots, fuser=fuser)
    assert lm_a.max_batch == 2 * slots
    kw = dict(cfg_coef=1.5, condition_tensors={"c": (cond, None)})
    manual = bc.ManualLoop(mimi_b, lm_b, slots, **kw)
    first = [f"s{i:02d}" for i in range(36)]
    script = [(0, "open", s) for s in first] + [(2, "close", "s33"), (2, "close", "s34"), (3, "open", "t0"), (3, "open", "t1"),
                                                (4, "skip", "s35")]
    with SessionBatcher(mimi_a, lm_a, slots, use_sampling=False, **kw) as batcher:
        assert batcher.total_slots == slots
        res, ref = bc.scripted_run(batcher, manual, mcfg.frame_size, script=script, n_steps=6)
    manual.stop()
    assert rows_launches(lm_a) > 0
    assert len(res["t0"]) > 0 and len(res["s35"]) > 0 and sum(len(v) for v in res.values()) > 100
    for s in res:
        assert len(res[s]) == len(ref[s]), f"session {s}: {len(res[s])} frames from the batcher, {len(ref[s])} by hand"
        for i, ((pa, ta), (pb, tb)) in enumerate(zip(res[s], ref[s])):
            assert np.array_equal(ta, tb), f"session {s} frame {i}: tokens differ"
            assert np.array_equal(pa, pb), f"session {s} frame {i}: PCM differs"


# ---- 8. refusals and the entry points ----------------------------------------------------------------------------------------------------
def check_refusals_and_api(device, lib):
    import pytest
    from moshi_amd.weights import quantize_lm_state_dict, quantize_lm_state_dict_fp8
    cfg = tiny_lm_config()
    sd = cached_lm_state_dict(cfg, 21)
    with pytest.raises(NotImplementedError, match="max_rows > 128"):
        LMModel(sd, cfg, device=device, max_rows=129, lib=lib)
    with pytest.raises(NotImplementedError, match="int8 / fp8 linears"):
        LMModel(quantize_lm_state_dict(sd), cfg, device=device, max_rows=96, lib=lib)
    with pytest.raises(NotImplementedError, match="int8 / fp8 linears"):
        LMModel(quantize_lm_state_dict_fp8(sd), cfg, device=device, max_rows=96, lib=lib)
    with pytest.raises(NotImplementedError, match="max_batch > 64"):
        LMModel(sd, cfg, device=device, max_batch=65, lib=lib)
    with pytest.raises(ValueError, match="mutually exclusive"):
        LMModel(sd, cfg, device=device, max_batch=65, max_rows=96, lib=lib)

    def launches(**kw):
        gen = LMGen(LMModel(sd, cfg, device=device, lib=lib, **kw), use_sampling=False, support_out_of_sync=True)
        with gen.streaming(64):
            out = gen.step_with_taps(torch.zeros(64, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=device))
            return [f"{a}\t{b}" for a, b in gen.launch_list()], [t.cpu() for t in out], rows_launches(gen)
    la, oa, ra = launches(max_rows=64)
    lb, ob, rb = launches(max_batch=64)
    assert la == lb and len(la) > 20 and ra == rb == 0
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    lm = LMModel(sd, cfg, device=device, max_rows=65, lib=lib)
    assert lm.max_batch == 65
    gen = LMGen(lm, use_sampling=False)
    with pytest.raises(AssertionError, match="exceeds max_batch"):
        gen.streaming_forever(66)
    with pytest.raises(NotImplementedError, match="not selected above 64 rows"):
        lm.debug_linear("depformer.layers.0.self_attn.in_projs.0.weight", torch.zeros(65, cfg.depformer_dim), path="norm_fused",
                        alpha_name="depformer.layers.0.norm1.alpha")


def check_control_equals_kernel(device, lib, B=97):
    """MMI_ROWS_GROUPS=1 (the A/B control: the <= 64-row kernels once per row group) computes the same network: text and audio
    logits inside the bf16 gate of lm_cases, greedy picks equal except at near ties (the control's K partition is that of the
    <= 64-row kernels: not bit-identical, so the two free-running streams are compared step by step only while the ring holds
    the same tokens - the inputs are forced by the delay ring's first steps)."""
    cfg = tiny_lm_config()
    sd = cached_lm_state_dict(cfg, 21)
    rng = np.random.default_rng(3)
    codes = [torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device) for _ in range(3)]

    def run(**knobs):
        with env(**knobs):
            lm = LMModel(sd, cfg, device=device, max_rows=B, lib=lib)
        gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
        with gen.streaming(B):
            out = [[t.float().cpu().numpy() for t in gen.step_with_taps(c)] for c in codes]
            return out, {k for _, k in gen.launch_list()}
    a, ka = run()
    b, kb = run(MMI_ROWS_GROUPS=1)
    assert "k_gemm_rows" in ka and kb & {"k_gemm_xp", "k_gemm_xlds"}, (ka, kb)
    cfg_q = cfg.dep_q
    for s in range(len(codes)):
        for r in range(B):
            assert lc.logits_close(b[s][1][r], a[s][1][r]), f"step {s} row {r}: text logits"
            for k in range(cfg_q):
                assert lc.logits_close(b[s][2][r, k], a[s][2][r, k]), f"step {s} row {r} cb {k}: audio logits"
                ta, tb = int(a[s][2][r, k].argmax()), int(b[s][2][r, k].argmax())
                assert ta == tb or lc.near_tie(a[s][2][r, k], ta, tb), f"step {s} row {r} cb {k}: greedy tokens part away from a tie"
