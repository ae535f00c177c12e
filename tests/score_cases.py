"""Cases for teacher-forced scoring on the prefill path (`mmi_lm_score` / `LMGen.score`), shared by the simulator suite
(tests/test_score_sim.py) and the MI355X suite (tests/test_b_score_gpu.py).

Part A holds the output kernel ALONE (`LMModel.debug_score_rows`: k_score_logprob through the launch function of a scoring pass) to
numpy in float64 on the same bf16 values.

LOGP_TOL = 2^-13 is derived, not measured: the kernel's sum of expf(x - max) is at most 128 terms per thread in ascending order plus a
tree of 6 + 2 additions, every rounding 2^-24 relative on positive terms - about 8e-6 in the logarithm; the device expf / logf add
a few ulp at magnitudes <= log(32768) = 10.4; the final difference (x_t - max) - log(sum) has a magnitude below 256 for logits
bounded by 64 (ulp 1.5e-5).  Under 3e-5 in total; 2^-13 = 1.2e-4 leaves 4 x.

Part B holds the call to its definition - the forced steps of `mmi_lm_prefill`'s definition, with what their parity taps return -
through the numpy oracle under the gates the stepped engine is held to (lm_cases.logits_close / near_tie, imported unchanged)."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config, tiny_stt_config
from moshi_amd.lm import ConditionFuser, LMGen, LMModel, ScoreOutput
from oracle.lm_oracle import LMOracle
from tests import lm_cases as lc
from tests import prefill_cases as pc
from tests.lm_cases import cached_lm_state_dict

LOGP_TOL = 2.0 ** -13
WIDTHS = (8, 2056, 2048, 32000)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 values rounded to the nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def logp64(rows: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """float64 log softmax(rows)[targets]; -inf where the target lies outside the row."""
    x = rows.astype(np.float64)
    m = x.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]
    inside = (targets >= 0) & (targets < rows.shape[-1])
    xt = np.take_along_axis(x, np.where(inside, targets, 0)[..., None], -1)[..., 0]
    return np.where(inside, xt - lse, -np.inf)


# ==== Part A: the output kernel ===========================================================================================================
def crafted_rows(N: int):
    """(rows fp32 [R, N] of bf16 values bounded by 64, targets int32 [R], names)."""
    rng = np.random.default_rng([N, 77])
    rows, tgt, names = [], [], []

    def add(name, row, t):
        rows.append(bf16_round(np.asarray(row, np.float32)))
        tgt.append(t)
        names.append(name)
    for v in (0.0, -37.5, 64.0):
        add(f"flat {v}", np.full(N, v), int(rng.integers(N)))
    hot = int(rng.integers(N))
    dom = np.full(N, -20.0)
    dom[hot] = 30.0
    add("dominant, target on it", dom, hot)
    add("dominant, target off it", dom, (hot + 1) % N)
    peak = rng.standard_normal(N).astype(np.float32) * 4
    peak[hot] = 64.0
    add("random under one peak at the bound", np.clip(peak, -64, 64), (hot + N // 2) % N)
    for lo, hi in ((0, N - 1), (N - 1, 0), (N // 2, N // 2 + 1) if N > 8 else (3, 4)):
        lo, hi = min(lo, hi), max(lo, hi)
        tie = bf16_round(rng.standard_normal(N).astype(np.float32))
        tie[[lo, hi]] = np.float32(tie.max() + 1.5)
        add(f"two-way tie of the maximum at {lo} and {hi}", tie, hi)
    for i, scale in enumerate((1.0, 8.0, 0.05, 20.0)):
        r = np.clip(rng.standard_normal(N).astype(np.float32) * scale, -64, 64)
        add(f"random x {scale}", r, int(rng.integers(N)))
        add(f"random x {scale}, first / last entry", r, 0 if i % 2 else N - 1)
    add("target == N", rng.standard_normal(N), N)
    add("target == N + 5", rng.standard_normal(N), N + 5)
    return np.stack(rows), np.asarray(tgt, np.int32), names


def check_output_kernel(lm, N: int):
    rows, tgt, names = crafted_rows(N)
    assert np.abs(rows).max() <= 64 and np.array_equal(bf16_round(rows), rows)
    t = torch.from_numpy(rows).to(torch.bfloat16)
    logp, am, wide = (x.cpu().numpy() for x in lm.debug_score_rows(t, torch.from_numpy(tgt)))
    again = tuple(x.cpu().numpy() for x in lm.debug_score_rows(t, torch.from_numpy(tgt)))
    want = logp64(rows, tgt.astype(np.int64))
    worst = 0.0
    for r, name in enumerate(names):
        if np.isinf(want[r]):
            assert logp[r] == -np.inf, f"N={N} {name}: logp {logp[r]!r}, the target lies outside the row"
        else:
            err = abs(float(logp[r]) - want[r])
            worst = max(worst, err)
            assert err <= LOGP_TOL, f"N={N} {name}: logp {logp[r]!r} against {want[r]!r} ({err:.3g} > 2^-13)"
        assert am[r] == int(np.argmax(rows[r])), f"N={N} {name}: argmax {am[r]} against {int(np.argmax(rows[r]))}"
    print(f"N={N}: worst |logp - logp64| = {worst:.3g} (bound {LOGP_TOL:.3g})")
    for v in (0.0, -37.5, 64.0):                                      # the flat rows: -log N
        r = names.index(f"flat {v}")
        assert abs(float(logp[r]) + np.log(N)) <= LOGP_TOL
    assert np.array_equal(wide.view(np.uint32), rows.view(np.uint32)), f"N={N}: the fp32 copy is not the bf16 row widened"
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((logp, am, wide), again)), f"N={N}: two launches differ"
    # one NaN entry: that row's logp is NaN, the rows next to it are what they were
    bad = rows.copy()
    r_nan = names.index("random x 1.0")
    bad[r_nan, N // 3] = np.nan
    lp2, _, _ = (x.cpu().numpy() if x is not None else None for x in lm.debug_score_rows(torch.from_numpy(bad).to(torch.bfloat16), torch.from_numpy(tgt),
                                                                                          want_f32=False))
    assert np.isnan(lp2[r_nan]), f"N={N}: a NaN logit gave logp {lp2[r_nan]!r}"
    keep = np.arange(len(names)) != r_nan
    assert np.array_equal(lp2[keep].view(np.uint32), logp[keep].view(np.uint32))


# ==== Part B: the call ====================================================================================================================
def score_model(device, lib, cfg, rows=32, prefill_rows=32, seed=21, score=True, **kw):
    return pc.model(device, lib, cfg, rows=rows, prefill_rows=prefill_rows, seed=seed, score=score, **kw)


def arrays(out: ScoreOutput):
    """The four outputs as numpy (None stays None)."""
    return tuple(None if t is None else np.ascontiguousarray(t.cpu().numpy()) for t in (out.logp, out.argmax, out.text_logits, out.audio_logits))


def check_self_consistent(out: ScoreOutput, toks: np.ndarray, what: str):
    """Case 3: logp is the float64 log-softmax of the call's own logits at the given token within 2^-13; argmax is np.argmax of them."""
    logp, am, tl, al = arrays(out)
    n, sites, T = toks.shape
    assert logp.shape == (n, sites, T) and am.shape == (n, sites, T) and logp.dtype == np.float32 and am.dtype == np.int64
    want = logp64(tl, toks[:, 0])                                     # [n, T]
    err = np.abs(logp[:, 0] - want)
    assert (err <= LOGP_TOL).all(), f"{what}: text logp off its own logits by {err.max():.3g}"
    assert np.array_equal(am[:, 0], tl.argmax(-1)), f"{what}: text argmax is not the argmax of the returned logits"
    if sites > 1:
        want = logp64(al, toks[:, 1:].transpose(0, 2, 1))             # [n, T, dep_q]
        err = np.abs(logp[:, 1:].transpose(0, 2, 1) - want)
        assert (err <= LOGP_TOL).all(), f"{what}: audio logp off its own logits by {err.max():.3g}"
        assert np.array_equal(am[:, 1:].transpose(0, 2, 1), al.argmax(-1)), f"{what}: audio argmax is not the argmax of the returned logits"
    else:
        assert al is None
    return float(err.max())


def oracle_frames(orc, cfg, B, T, seed):
    """The oracle steps T greedy frames: (codes [B, n_user, T], its stored tokens [B, 1 + dep_q, T], text logits [B, T, text_card],
    audio logits [B, T, dep_q, card])."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, T)).astype(np.int64)
    toks = np.zeros((B, 1 + cfg.dep_q, T), np.int64)
    otl = np.zeros((B, T, cfg.text_card), np.float32)
    oal = np.zeros((B, T, cfg.dep_q, cfg.card), np.float32)
    for f in range(T):
        _, (tl, al, tt, at) = orc.step(codes[:, :, f:f + 1], use_sampling=False, support_out_of_sync=True)
        toks[:, 0, f] = tt
        otl[:, f] = tl
        if cfg.dep_q:
            toks[:, 1:, f] = at
            oal[:, f] = al
    return codes, toks, otl, oal


def check_against_oracle(out: ScoreOutput, toks, otl, oal, what):
    """Case 2: every (session, frame, site) under logits_close against the oracle's logits of that step; argmax equal or a near tie."""
    _, am, tl, al = arrays(out)
    B, sites, T = toks.shape
    for b in range(B):
        for f in range(T):
            assert lc.logits_close(tl[b, f], otl[b, f]), f"{what} session {b} frame {f}: text logits {np.abs(tl[b, f] - otl[b, f]).max()}"
            t_e, t_o = int(am[b, 0, f]), int(toks[b, 0, f])
            assert t_e == t_o or lc.near_tie(otl[b, f], t_e, t_o), f"{what} session {b} frame {f}: text argmax {t_e} against {t_o}"
            for k in range(sites - 1):
                assert lc.logits_close(al[b, f, k], oal[b, f, k]), f"{what} session {b} frame {f} cb {k}: {np.abs(al[b, f, k] - oal[b, f, k]).max()}"
                a_e, a_o = int(am[b, 1 + k, f]), int(toks[b, 1 + k, f])
                assert a_e == a_o or lc.near_tie(oal[b, f, k], a_e, a_o), f"{what} session {b} frame {f} cb {k}: argmax {a_e} against {a_o}"


def check_score_vs_oracle(device, lib, kind="moshi", prefill_rows=128, kv="bf16", cond=False, cfg=None, B=3, starts=(0, 9, 30), T=23, seed=901,
                          rows=32, want_rows_gemm=False):
    """Cases 2 and 3 (and 8 with `cfg`): B sessions moved to `starts` (the tiny context is 12: two of them wrap) score T frames with
    commit = 1 and return_logits; the oracle steps the same frames greedily, its stored tokens are the `tokens` argument."""
    if cfg is None:
        cfg = tiny_lm_config() if kind == "moshi" else tiny_stt_config()
    if kv != "bf16":
        cfg = replace(cfg, kv_cache_dtype=kv)
    sd = cached_lm_state_dict(cfg, seed)
    kw, okw = {}, {}
    if cond:
        rng = np.random.default_rng(seed)
        cs = torch.from_numpy(0.5 * rng.standard_normal((B, 1, cfg.dim)).astype(np.float32)).to(torch.bfloat16)
        kw = dict(fuser=ConditionFuser({"sum": ["c"]}))
        okw = dict(condition_tensors={"c": (cs, None)})
    size = dict(max_rows=rows) if rows > 64 else dict(max_batch=rows)
    lm = LMModel(sd, cfg, device=device, lib=lib, prefill_rows=prefill_rows, score=True, **size, **kw)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, **okw)
    if kv == "fp4":
        from tests.kv4_cases import Kv4Oracle
        orc = Kv4Oracle(sd, cfg)
    else:
        orc = LMOracle(sd, cfg)
    if cond:
        orc.streaming(B, condition_sum=cs.float().numpy().reshape(B, cfg.dim))
    else:
        orc.streaming(B)
    orc.seek(list(starts))
    codes, toks, otl, oal = oracle_frames(orc, cfg, B, T, seed + 1)
    what = f"{kind} {kv} ring, prefill_rows {prefill_rows}" + (", sum condition" if cond else "")
    with gen.streaming(B):
        gen.seek(list(starts))
        out = gen.score(torch.from_numpy(codes), torch.from_numpy(toks), commit=True, return_logits=True)
        offs = pc.state_of(gen)["offsets"].view(np.int64)[:, 0]
        rows_launches = int(gen._lib.mmi_lm_stat(lm._handle, 4))
    assert np.array_equal(offs, np.asarray(starts) + T), f"{what}: commit = 1 left the offsets at {offs}"
    if want_rows_gemm:
        assert rows_launches > 0, "no linear of the pass ran k_gemm_rows"
    check_against_oracle(out, toks, otl, oal, what)
    worst = check_self_consistent(out, toks, what)
    print(f"{what}: worst |logp - logp64(own logits)| = {worst:.3g}")


def head_width_config():
    """Case 8: the head widths and the depth transformer's width the tiny models do not reach."""
    return replace(tiny_lm_config(), card=2048, text_card=32000, depformer_dim=1024, depformer_num_heads=16, depformer_dim_feedforward=4224,
                   depformer_num_layers=1)


def schedule_config():
    """A depformer weight schedule without low-rank tables: micro-steps 1 .. 7 share one weight set."""
    return replace(tiny_lm_config(), depformer_weights_per_step_schedule=[0] + [1] * 7)


def check_score_vs_forced_steps(device, lib, cfg, B=2, T=9, prefill_rows=32, seed=21):
    """The definition without the oracle (which has no weight schedule): a twin steps the same frames one by one with the tokens forced;
    the parity taps of step f are the reference of frame f under the same gates."""
    codes, toks = pc.frames(cfg, B, T, 3)
    gen = LMGen(score_model(device, lib, cfg, rows=8, prefill_rows=prefill_rows, seed=seed), use_sampling=False, support_out_of_sync=True)
    with gen.streaming(B):
        out = gen.score(torch.from_numpy(codes), torch.from_numpy(toks), return_logits=True)
    twin = LMGen(score_model(device, lib, cfg, rows=8, prefill_rows=None, seed=seed, score=False), use_sampling=False, support_out_of_sync=True)
    stl = np.zeros((B, T, cfg.text_card), np.float32)
    sal = np.zeros((B, T, cfg.dep_q, cfg.card), np.float32)
    with twin.streaming(B):
        for f in range(T):
            _, tl, al = twin.step_with_taps(torch.from_numpy(codes[:, :, f:f + 1]).to(device), forced_tokens=torch.from_numpy(toks[:, :, f]).to(device))
            stl[:, f], sal[:, f] = tl.cpu().numpy(), al.cpu().numpy()
    _, am, tl, al = arrays(out)
    for b in range(B):
        for f in range(T):
            assert lc.logits_close(tl[b, f], stl[b, f]), f"session {b} frame {f}: text logits"
            assert am[b, 0, f] == stl[b, f].argmax() or lc.near_tie(stl[b, f], int(am[b, 0, f]), int(stl[b, f].argmax()))
            for k in range(cfg.dep_q):
                assert lc.logits_close(al[b, f, k], sal[b, f, k]), f"session {b} frame {f} cb {k}: audio logits"
                assert am[b, 1 + k, f] == sal[b, f, k].argmax() or lc.near_tie(sal[b, f, k], int(am[b, 1 + k, f]), int(sal[b, f, k].argmax()))
    check_self_consistent(out, toks, "weight schedule")


def check_commit_is_prefill(device, lib, kv="bf16", starts=(3, 0, 30), named=(0, 2, 3), B=5, T=23, prefill_rows=16):
    """Case 4: a handle scored with commit = 1 and a twin prefilled with the same arguments: identical on the named sessions, every ring
    included; the others equal their state before the call."""
    cfg = replace(tiny_lm_config(), kv_cache_dtype=kv) if kv != "bf16" else tiny_lm_config()
    n = len(named)
    codes, toks = pc.frames(cfg, n, T, 5)
    offs = [0] * B
    for s, o in zip(named, starts):
        offs[s] = o
    res = {}
    for how in ("score", "prefill"):
        gen = LMGen(score_model(device, lib, cfg, rows=8, prefill_rows=prefill_rows, score=how == "score"), use_sampling=False, support_out_of_sync=True)
        with gen.streaming(B):
            gen.seek(offs)
            before = pc.state_of(gen)
            if how == "score":
                out = gen.score(torch.from_numpy(codes), torch.from_numpy(toks), sessions=named, commit=True)
                assert out.text_logits is None and out.audio_logits is None and np.isfinite(out.logp.cpu().numpy()).all()
            else:
                gen.prefill(torch.from_numpy(codes), torch.from_numpy(toks), sessions=named)
            res[how] = (before, pc.state_of(gen))
    others = [b for b in range(B) if b not in named]
    pc.compare_states(res["score"][0], res["score"][1], others, f"{kv} ring: sessions not named, against their state before the score", rings="all")
    pc.compare_states(res["score"][1], res["prefill"][1], list(named), f"{kv} ring: score(commit=1) against prefill", rings="all")
    pc.compare_states(res["score"][1], res["prefill"][1], None, f"{kv} ring: score(commit=1) against prefill, every session", rings="all")


def full_state(gen):
    """(the whole state buffer, the kind-1 regions by name with rng in full)."""
    buf = gen.get_streaming_state()["lm_gen"].cpu().numpy().copy()
    named = {}
    for name, (off, nbytes, rows, kind) in gen.state_regions().items():
        if kind == 1:
            named[name] = buf[off:off + nbytes].copy()
    return buf, named


def check_commit0_leaves_no_trace(device, lib, kv="bf16", B=4, named=(1, 3), T=10, prefill_rows=32):
    """Case 5."""
    cfg = replace(tiny_lm_config(), kv_cache_dtype=kv) if kv != "bf16" else tiny_lm_config()
    n_user = cfg.n_q - cfg.dep_q
    rng = np.random.default_rng(12)
    live = [torch.from_numpy(rng.integers(0, cfg.card, (B, n_user, 1))).to(device) for _ in range(16)]
    codes, toks = pc.frames(cfg, len(named), T, 6)
    res = {}
    for how in ("scored", "twin"):
        gen = LMGen(score_model(device, lib, cfg, rows=8, prefill_rows=prefill_rows), use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10,
                    seed=5, support_out_of_sync=True)
        with gen.streaming(B):
            for c in live[:15]:                                       # 15 > the context of 12: the rings have wrapped
                gen.step(c)
            if how == "scored":
                buf0, named0 = full_state(gen)
                a = arrays(gen.score(torch.from_numpy(codes), torch.from_numpy(toks), sessions=named, commit=False, return_logits=True))
                buf1, named1 = full_state(gen)
                b = arrays(gen.score(torch.from_numpy(codes), torch.from_numpy(toks), sessions=named, commit=False, return_logits=True))
                for name in named0:
                    assert np.array_equal(named0[name], named1[name]), f"{kv} ring: commit = 0 changed region {name}"
                assert np.array_equal(buf0, buf1), f"{kv} ring: commit = 0 changed the state buffer ({int((buf0 != buf1).sum())} bytes)"
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), "a second identical call returned other bytes"
                assert np.isfinite(a[0]).all()
            out, tl, al = gen.step_with_taps(live[15])
            res[how] = (out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy())
    for x, y, what in zip(res["scored"], res["twin"], ("tokens", "text logits", "audio logits")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{kv} ring: the step after a commit = 0 score differs from a twin that never scored ({what})"
    return a


def check_between_steps_of_a_live_batch(device, lib, B=8, picked=(2, 5), T=10):
    """Case 6."""
    cfg = tiny_lm_config()
    rng = np.random.default_rng(17)
    n_user = cfg.n_q - cfg.dep_q
    live = [torch.from_numpy(rng.integers(0, cfg.card, (B, n_user, 1))).to(device) for _ in range(9)]
    codes, toks = pc.frames(cfg, len(picked), T, 23)
    outs = {}
    for how in ("none", "commit0", "commit1"):
        gen = LMGen(score_model(device, lib, cfg, rows=B, prefill_rows=32), use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=5,
                    support_out_of_sync=True)
        got = []
        with gen.streaming(B):
            for c in live[:3]:
                gen.step(c)
            if how != "none":
                gen.score(torch.from_numpy(codes), torch.from_numpy(toks), sessions=picked, commit=how == "commit1")
            for c in live[3:]:
                got.append(gen.step(c)[:, :, 0].cpu().numpy())
        outs[how] = got
    others = [b for b in range(B) if b not in picked]
    for s in range(6):
        for how in ("commit0", "commit1"):
            assert np.array_equal(outs[how][s][others], outs["none"][s][others]), f"step {s} after score ({how}): a neighbour's tokens depend on it"
        assert np.array_equal(outs["commit0"][s], outs["none"][s]), f"step {s} after score (commit = 0): the scored sessions' tokens changed"
    assert any((o >= 0).all() for o in outs["none"]), "no step produced tokens: nothing shown"
    assert any(not np.array_equal(a[list(picked)], b[list(picked)]) for a, b in zip(outs["commit1"], outs["none"])), \
        "commit = 1 left the scored sessions where they were: nothing shown"


def check_refusals_and_off_state(device, lib):
    """Case 7."""
    import ctypes as C

    import pytest
    from moshi_amd import _capi
    from moshi_amd.lm import TTSMachine
    from moshi_amd.weights import quantize_lm_state_dict
    cfg = tiny_lm_config()
    sd = cached_lm_state_dict(cfg, 21)
    n_user = cfg.n_q - cfg.dep_q
    # ---- at enable
    with pytest.raises(RuntimeError, match="mmi_lm_enable_prefill first"):
        LMModel(sd, cfg, device=device, lib=lib, max_batch=32, score=True)
    with pytest.raises(NotImplementedError, match="quantised linears"):
        LMModel(quantize_lm_state_dict(sd), cfg, device=device, lib=lib, max_batch=32, prefill_rows=32, score=True)
    with pytest.raises(NotImplementedError, match="adapter handles"):
        LMModel(sd, cfg, device=device, lib=lib, max_batch=32, adapters=(2, 32), prefill_rows=32, score=True)
    from tests import row_condition_cases as rcc
    xcfg = rcc.tiny_cross_config()
    with pytest.raises(NotImplementedError, match="cross-attention"):
        LMModel(cached_lm_state_dict(xcfg, 21), xcfg, device=device, lib=lib, max_batch=32, prefill_rows=32, score=True, fuser=ConditionFuser({"cross": ["x"]}))
    from tests.tts_cases import h_config
    lrcfg = h_config()
    with pytest.raises(NotImplementedError, match="low-rank or demuxed depformer embeddings"):
        LMModel(cached_lm_state_dict(lrcfg, 21), lrcfg, device=device, lib=lib, max_batch=32, prefill_rows=32, score=True)
    dmcfg = replace(cfg, demux_second_text_stream=True)
    with pytest.raises(NotImplementedError, match="low-rank or demuxed depformer embeddings"):
        LMModel(cached_lm_state_dict(dmcfg, 21), dmcfg, device=device, lib=lib, max_batch=32, prefill_rows=32, score=True)
    # ---- at the call
    codes, toks = pc.frames(cfg, 2, 3, 1)
    tc, tt = torch.from_numpy(codes), torch.from_numpy(toks)
    lm = LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=8, score=True)
    assert lm._lib.mmi_lm_score_enabled(lm._handle) == 1
    with pytest.raises(NotImplementedError, match="TTS machine"):
        LMGen(lm, use_sampling=False, tts_machine=TTSMachine(text_card=cfg.text_card + 1)).streaming_forever(2)
    lm._lib.check(lm._lib.mmi_lm_streaming_stop(lm._handle))
    gen = LMGen(lm, use_sampling=False, on_text_hook=lambda t: None)
    with gen.streaming(2):
        with pytest.raises(NotImplementedError, match="hooks"):
            gen.score(tc, tt)
    cs = torch.zeros(4, 1, cfg.dim, dtype=torch.bfloat16)
    glm = LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=8, score=True, fuser=ConditionFuser({"sum": ["c"]}))
    gen = LMGen(glm, use_sampling=False, cfg_coef=2.0, condition_tensors={"c": (cs, None)})
    with gen.streaming(2):
        with pytest.raises(NotImplementedError, match="guided"):
            gen.score(tc, tt)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    with pytest.raises(RuntimeError, match="streaming"):
        gen.score(tc, tt)
    with gen.streaming(3):
        gen.step(torch.zeros(3, n_user, 1, dtype=torch.int64).to(device))
        before = full_state(gen)[0]
        with pytest.raises(RuntimeError, match="not while streaming"):
            lm._lib.check(lm._lib.mmi_lm_enable_score(lm._handle, 0))
        with pytest.raises(ValueError, match="out of range"):
            gen.score(tc, tt, sessions=[0, 3])
        with pytest.raises(ValueError, match="named twice"):
            gen.score(tc, tt, sessions=[1, 1])
        with pytest.raises(ValueError, match="sessions per call"):
            gen.score(torch.zeros(9, n_user, 1, dtype=torch.int64), torch.zeros(9, 1 + cfg.dep_q, 1, dtype=torch.int64), sessions=[0, 1, 2] * 3)
        codes5, toks5 = pc.frames(cfg, 2, 5, 2)
        with pytest.raises(ValueError, match="commit = 0 must fit one pass"):
            gen.score(torch.from_numpy(codes5), torch.from_numpy(toks5), sessions=[0, 1], commit=False)      # 2 x 5 rows > 8
        gen.score(torch.from_numpy(codes5[:, :, :4]), torch.from_numpy(toks5[:, :, :4]), sessions=[0, 1], commit=False)   # 2 x 4 rows fit
        dc, dt = tc.to(device), tt.to(device)
        sess = (C.c_int32 * 2)(0, 1)
        logp = torch.empty(2, 3, 1 + cfg.dep_q, dtype=torch.float32, device=device)
        with pytest.raises(ValueError, match="T must be"):
            o = _capi.ScoreOut(logp.data_ptr(), None, None, None)
            lm._lib.check(lm._lib.mmi_lm_score(lm._handle, sess, 2, dc.data_ptr(), dt.data_ptr(), 0, 1, C.byref(o), None))
        with pytest.raises(ValueError, match="logp must not be null"):
            o = _capi.ScoreOut(None, None, None, None)
            lm._lib.check(lm._lib.mmi_lm_score(lm._handle, sess, 2, dc.data_ptr(), dt.data_ptr(), 3, 1, C.byref(o), None))
        with pytest.raises(ValueError, match="null argument"):
            lm._lib.check(lm._lib.mmi_lm_score(lm._handle, sess, 2, dc.data_ptr(), dt.data_ptr(), 3, 1, None, None))
        with pytest.raises(AssertionError, match="tokens must be"):
            LMGen.score(pc._checked(gen), tc, -tt - 1, sessions=[0, 1])
        assert np.array_equal(before, full_state(gen)[0]), "a refused call changed the state"
        # only logp asked for: the other three outputs are optional
        o = _capi.ScoreOut(logp.data_ptr(), None, None, None)
        lm._lib.check(lm._lib.mmi_lm_score(lm._handle, sess, 2, dc.data_ptr(), dt.data_ptr(), 3, 0, C.byref(o), None))
        assert np.isfinite(logp.cpu().numpy()).all()
    # ---- the off state: prefill without score is what it was
    rng = np.random.default_rng(2)
    steps = [torch.from_numpy(rng.integers(0, cfg.card, (2, n_user, 1))).to(device) for _ in range(3)]

    def run(score):
        m = LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=32, score=score)
        assert m._lib.mmi_lm_score_enabled(m._handle) == int(score)
        g = LMGen(m, use_sampling=True, seed=9, support_out_of_sync=True)
        with g.streaming(2):
            toks_ = [g.step(c)[:, :, 0].cpu().numpy() for c in steps]
            if not score:
                with pytest.raises(RuntimeError, match="score is not enabled"):
                    g.score(tc, tt)
                o = _capi.ScoreOut(logp.data_ptr(), None, None, None)
                with pytest.raises(RuntimeError, match="score is not enabled"):
                    m._lib.check(m._lib.mmi_lm_score(m._handle, (C.c_int32 * 2)(0, 1), 2, tc.to(device).data_ptr(), tt.to(device).data_ptr(), 3, 1,
                                                     C.byref(o), None))
            return [f"{a}\t{b}" for a, b in g.launch_list()], int(g._lib.mmi_lm_state_bytes(m._handle)), toks_
    off, on = run(False), run(True)
    assert off[0] == on[0], "the launch list of a step changed"
    assert off[1] == on[1], "mmi_lm_state_bytes changed"
    assert all(np.array_equal(x, y) for x, y in zip(off[2], on[2]))
    assert not any("k_sc_" in k or "score" in k for k in on[0])
