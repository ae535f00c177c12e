"""Cases for the log-probabilities of the live step (`mmi_lm_enable_logprobs` / `LMGen(logprobs=n)`), shared by the
simulator suite (tests/test_logprobs_sim.py) and the MI355X suite (tests/test_b_logprobs_gpu.py).

The reference of every value is the float64 log-softmax of the bf16 logits widened exactly; the ids are compared with a stable sort by
(-value, index), which is exact.  LOGP_TOL = 2^-13 is DESIGN 8.21's bound (tests/score_cases.py derives it): k_step_logprob forms the
maximum and the sum term for term as k_score_logprob does, which part A pins bit for bit against `LMModel.debug_score_rows`.

Part A holds the kernel alone (`LMModel.debug_step_logprob`: k_step_logprob through the step op's launch function on crafted rows);
B..E the op inside the step, against the tap applied to the step's own tap logits with `last_tokens()` as targets, bit for bit;
F the session batcher; G what the entry points refuse."""
from __future__ import annotations

import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch

from moshi_amd import _capi
from moshi_amd.batcher import SessionBatcher
from moshi_amd.config import tiny_lm_config, tiny_stt_config
from moshi_amd.lm import ConditionFuser, LMGen, LMModel
from tests import batcher_cases as bc
from tests.lm_cases import cached_lm_state_dict
from tests.score_cases import LOGP_TOL, bf16_round, logp64

WIDTHS = (8, 2048, 2056, 32000, 32768)
TOP_NS = (0, 1, 8)


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b) -> bool:
    return np.array_equal(bits(a), bits(b))


def ref_top(rows: np.ndarray, top_n: int):
    """(ids int64 [R, top_n], their float64 log-probabilities): the first top_n in the order (value descending, index ascending)."""
    x = rows.astype(np.float64)
    ids = np.argsort(-x, axis=-1, kind="stable")[:, :top_n]
    m = x.max(-1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(-1, keepdims=True))
    return ids, np.take_along_axis(x, ids, -1) - lse


def lp_arrays(lp):
    return lp.logp.cpu().numpy(), lp.top_ids.cpu().numpy(), lp.top_logp.cpu().numpy()


# ==== Part A: the kernel alone ============================================================================================================
def crafted_rows(N: int):
    """[(name, row fp32 of bf16 values bounded by 64, target)]: the families, the ties by construction, the targets."""
    rng = np.random.default_rng([N, 823])
    out = []

    def add(name, row, t):
        out.append((name, bf16_round(np.asarray(row, np.float32)), int(t)))
    rnd = np.clip(rng.standard_normal(N).astype(np.float32) * 6, -64, 64)
    order = np.argsort(-bf16_round(rnd), kind="stable")
    add("random, target the maximum (inside the alternatives)", rnd, order[0])
    add("random, target the smallest (outside the alternatives)", rnd, order[-1])
    add("random, target -1", rnd, -1)
    add("random, target N", rnd, N)
    add("flat", np.full(N, -3.25), N // 2)
    hot = int(rng.integers(N))
    dom = np.full(N, -20.0)
    dom[hot] = 60.0
    add("one entry 80 above the rest, target on it", dom, hot)
    add("one entry 80 above the rest, target off it", dom, (hot + 1) % N)
    add("falling ramp (runs of equal bf16 values)", 32.0 - np.arange(N) * (64.0 / N), min(N - 1, 11))
    # two equal maxima: in one piece, in two pieces of one thread, in two waves
    for what, (i, j) in (("one piece", (5, 6)), ("two pieces of one thread", (5, 8 * 256 + 5)), ("two waves", (5, 8 * 64 + 5))):
        if j >= N:
            continue
        tie = bf16_round(rng.standard_normal(N).astype(np.float32))
        tie[[i, j]] = np.float32(tie.max() + 1.5)
        add(f"two equal maxima in {what} ({i}, {j})", tie, j)
    base = bf16_round(rng.standard_normal(N).astype(np.float32))
    top8 = np.float32(base.max()) + np.asarray([3, 7, 1, 8, 2, 6, 4, 5], np.float32)       # distinct, not in index order
    p0 = base.copy()
    p0[:8] = top8
    add("the eight largest all in piece 0", p0, 3)
    threads = (3, 40, 70, 100, 130, 170, 200, 250)                                          # two per wave, four waves
    if 8 * threads[-1] + 8 <= N:
        spread = base.copy()
        spread[[8 * t + t % 8 for t in threads]] = top8
        add("the eight largest one per piece of eight threads over four waves", spread, 8 * threads[2] + threads[2] % 8)
    return out


def check_tap_rows(lm, rows: np.ndarray, tgt: np.ndarray, top_n: int, names, what: str):
    """One tap launch on `rows` against float64, and bit for bit against k_score_logprob with the ids as targets."""
    R, N = rows.shape
    assert np.abs(rows).max() <= 64 and np.array_equal(bf16_round(rows), rows)
    t = torch.from_numpy(rows).to(torch.bfloat16)
    tg = torch.from_numpy(tgt.astype(np.int32))
    logp, ids, tlp = lp_arrays(lm.debug_step_logprob(t, tg, top_n))
    again = lp_arrays(lm.debug_step_logprob(t, tg, top_n))
    assert logp.shape == (R,) and ids.shape == (R, top_n) and tlp.shape == (R, top_n) and ids.dtype == np.int64
    assert all(same_bits(a, b) for a, b in zip((logp, ids, tlp), again)), f"{what}: two launches differ"
    want = logp64(rows, tgt.astype(np.int64))
    want_ids, want_tlp = ref_top(rows, top_n)
    worst = 0.0
    for r in range(R):
        if np.isinf(want[r]):
            assert logp[r] == -np.inf, f"{what} {names[r]}: logp {logp[r]!r}, the target lies outside the row"
        else:
            worst = max(worst, abs(float(logp[r]) - want[r]))
            assert abs(float(logp[r]) - want[r]) <= LOGP_TOL, f"{what} {names[r]}: logp {logp[r]!r} against {want[r]!r}"
        assert np.array_equal(ids[r], want_ids[r]), f"{what} {names[r]}: ids {ids[r].tolist()} against {want_ids[r].tolist()}"
        err = np.abs(tlp[r].astype(np.float64) - want_tlp[r])
        worst = max([worst] + err.tolist())
        assert (err <= LOGP_TOL).all(), f"{what} {names[r]}: top_logp off by {err.max():.3g}"
    # bit identity with the scoring kernel: the same row, the same target
    s_logp, s_am, _ = (x.cpu().numpy() if x is not None else None for x in lm.debug_score_rows(t, tg, want_f32=False))
    assert same_bits(logp, s_logp), f"{what}: logp is not k_score_logprob's, bit for bit"
    for k in range(top_n):
        k_logp, _, _ = lm.debug_score_rows(t, torch.from_numpy(ids[:, k].astype(np.int32)), want_f32=False)
        assert same_bits(tlp[:, k], k_logp.cpu().numpy()), f"{what}: top_logp[{k}] is not k_score_logprob's at that id"
    if top_n:
        assert np.array_equal(ids[:, 0], s_am), f"{what}: top_id[0] is not k_score_logprob's argmax"
    return worst


def check_kernel(lm, N: int, top_ns=TOP_NS):
    cases = crafted_rows(N)
    names = [c[0] for c in cases]
    rows = np.stack([c[1] for c in cases])
    tgt = np.asarray([c[2] for c in cases], np.int64)
    worst = 0.0
    for top_n in top_ns:
        for r0 in range(0, len(cases), 3):                      # three rows per launch, the last launch what is left
            sl = slice(r0, r0 + 3)
            worst = max(worst, check_tap_rows(lm, rows[sl], tgt[sl], top_n, names[sl], f"N={N} top_n={top_n}"))
        worst = max(worst, check_tap_rows(lm, rows[:1], tgt[:1], top_n, names[:1], f"N={N} top_n={top_n} (one row)"))
    print(f"N={N}: worst |logp - float64| = {worst:.3g} (bound {LOGP_TOL:.3g})")


def tie_digest(lm, N: int = 2056) -> bytes:
    """The bytes of the tie cases (A.3) at top_n = 8, checked - for runs under other workgroup schedules."""
    cases = [c for c in crafted_rows(N) if "equal maxima" in c[0] or "eight largest" in c[0]]
    assert len(cases) == 5
    rows, tgt = np.stack([c[1] for c in cases]), np.asarray([c[2] for c in cases], np.int64)
    check_tap_rows(lm, rows, tgt, 8, [c[0] for c in cases], f"N={N} ties")
    out = lp_arrays(lm.debug_step_logprob(torch.from_numpy(rows).to(torch.bfloat16), torch.from_numpy(tgt.astype(np.int32)), 8))
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


# ==== Part B: in the step =================================================================================================================
def tiny_model(device, lib, n, cfg=None, seed=21, **kw):
    cfg = cfg or tiny_lm_config()
    if "max_rows" not in kw:
        kw.setdefault("max_batch", n)
    return cfg, LMModel(cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), seed), cfg, device=device, lib=lib, **kw)


def user_codes(cfg, n, steps, device, seed=9):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, cfg.card, (n, cfg.n_q - cfg.dep_q, 1))).to(device) for _ in range(steps)]


def tap_of_step(gen, tl, al, toks: np.ndarray, rows, top_n):
    """The tap applied to the step's tap logits of `rows` with their stored tokens as targets: (logp [r, S], ids [r, S, n], top_logp)."""
    lm, q = gen.lm_model, gen.lm_model.dep_q
    rows = list(rows)
    a = lp_arrays(lm.debug_step_logprob(tl[rows].to(torch.bfloat16), torch.from_numpy(toks[rows, 0].astype(np.int32)), top_n))
    parts = [tuple(x[:, None] for x in a)]
    if q:
        card = al.shape[-1]
        b = lp_arrays(lm.debug_step_logprob(al[rows].reshape(-1, card).to(torch.bfloat16),
                                            torch.from_numpy(toks[rows, 1:].reshape(-1).astype(np.int32)), top_n))
        parts.append((b[0].reshape(len(rows), q), b[1].reshape(len(rows), q, top_n), b[2].reshape(len(rows), q, top_n)))
    return tuple(np.concatenate([p[i] for p in parts], 1) for i in range(3))


def assert_last_is_tap(gen, tl, al, rows, top_n, what):
    """last_logprobs() of the executed `rows` equals the tap on this step's tap logits, bit for bit, and float64 within 2^-13."""
    toks = gen.last_tokens().cpu().numpy()
    got = lp_arrays(gen.last_logprobs())
    want = tap_of_step(gen, tl, al, toks, rows, top_n)
    for g, w, name in zip(got, want, ("logp", "top_ids", "top_logp")):
        assert same_bits(g[list(rows)], w), f"{what}: {name} of the step is not the tap on the step's own logits"
    x = tl[list(rows)].cpu().numpy()
    ref = logp64(x, toks[list(rows), 0])
    fin = np.isfinite(ref)
    assert (np.abs(got[0][list(rows), 0][fin] - ref[fin]) <= LOGP_TOL).all() and (got[0][list(rows), 0][~fin] == -np.inf).all(), what
    return toks, got


def assert_nothing_recorded(vals, where, what):
    logp, ids, tlp = vals
    assert np.isnan(logp[where]).all() and (ids[where] == -1).all() and np.isnan(tlp[where]).all(), f"{what}: expected NaN / -1"


def check_in_step(device, lib, cfg=None, n=3, steps=None, top_n=3, seed=5):
    """Seeded sampling through step_with_taps under an exec mask (from the second step on) and one partial reset; both read-outs
    after every step."""
    cfg, lm = tiny_model(device, lib, n, cfg)
    D, delays, q = cfg.max_delay, list(cfg.delays), cfg.dep_q
    steps = steps or D + 6
    codes = user_codes(cfg, n, steps, device)
    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=0.8, seed=seed, support_out_of_sync=True, logprobs=top_n)
    reset_at = next(s for s in range(max(1, steps // 2), steps) if s % n == 1)      # row 1 is reset at a step that masks it out
    n_exec = [0] * n
    rec = [dict() for _ in range(n)]                # per row: executed step number -> (its step-coordinate values, its tokens)
    hidden = shown = 0
    with gen.streaming(n):
        prev = lp_arrays(gen.last_logprobs())
        assert_nothing_recorded(prev, np.ones(n, bool), "before the first step")
        for s in range(steps):
            ex = np.asarray([s == 0 or b != s % n for b in range(n)])
            if s == reset_at:
                m = np.zeros(n, bool)
                m[1] = True
                gen.reset_streaming(torch.from_numpy(m))
                n_exec[1], rec[1] = 0, {}
                after = lp_arrays(gen.last_logprobs())
                assert_nothing_recorded(after, m, f"step {s}: the reset row")
                assert all(same_bits(a[~m], p[~m]) for a, p in zip(after, prev)), f"step {s}: the reset touched another row"
                prev = after
            gen.set_exec_mask(torch.from_numpy(ex))
            out, tl, al = gen.step_with_taps(codes[s])
            out = out.cpu().numpy()[:, :, 0]
            rows = np.flatnonzero(ex)
            toks, got = assert_last_is_tap(gen, tl, al, rows, top_n, f"step {s}")
            assert all(same_bits(g[~ex], p[~ex]) for g, p in zip(got, prev)), f"step {s}: a masked row changed"
            prev = got
            for b in rows:
                n_exec[b] += 1
                rec[b][n_exec[b]] = (tuple(g[b].copy() for g in got), toks[b].copy())
            fr = lp_arrays(gen.frame_logprobs())
            for b in range(n):
                for c in range(1 + q):
                    if out[b, c] == -2:
                        assert_nothing_recorded(tuple(f[b, c] for f in fr), Ellipsis, f"step {s} frame ({b}, {c})")
                        hidden += 1
                        continue
                    vals, tk = rec[b][n_exec[b] - (D - delays[c])]
                    assert tk[c] == out[b, c], f"step {s} frame ({b}, {c}): the test's own bookkeeping is off"
                    assert all(same_bits(f[b, c], v[c]) for f, v in zip(fr, vals)), f"step {s} frame ({b}, {c}): not the values of the step that sampled it"
                    assert np.isfinite(fr[0][b, c]) or fr[0][b, c] == -np.inf
                    shown += 1
    assert hidden > 0 and shown > 0 and n_exec[1] < n_exec[0]


# ==== Part C: forcing and hooks ===========================================================================================================
def check_forcing_and_hooks(device, lib, n=2, top_n=2):
    cfg, lm = tiny_model(device, lib, n)
    codes = user_codes(cfg, n, 3, device)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, logprobs=top_n)
    with gen.streaming(n):
        forced = torch.full((n, 1 + cfg.dep_q), -1, dtype=torch.int64)
        forced[:, 0] = cfg.text_card                              # the initial-token id: outside the head's range
        _, tl, al = gen.step_with_taps(codes[0], forced_tokens=forced)
        toks, got = assert_last_is_tap(gen, tl, al, range(n), top_n, "forced text token")
        assert (toks[:, 0] == cfg.text_card).all() and (got[0][:, 0] == -np.inf).all() and np.isfinite(got[0][:, 1:]).all()
        _, tl, al = gen.step_with_taps(codes[1])                  # forcing holds for one step
        _, got = assert_last_is_tap(gen, tl, al, range(n), top_n, "the step after")
        assert np.isfinite(got[0]).all()
    swap = 7

    def on_text(t):
        t[:] = swap
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, logprobs=top_n, on_text_hook=on_text)
    with gen.streaming(n):
        for s in range(2):
            _, tl, al = gen.step_with_taps(codes[s])
            toks, got = assert_last_is_tap(gen, tl, al, range(n), top_n, f"hooked step {s}")
            assert (toks[:, 0] == swap).all()
            x = tl.cpu().numpy()
            assert (np.abs(got[0][:, 0] - logp64(x, np.full(n, swap))) <= LOGP_TOL).all(), "logp is not the replaced token's"
            assert np.array_equal(got[1][:, 0], ref_top(x, top_n)[0]), "the alternatives are not those of the text logits"


# ==== Part D: other handles ===============================================================================================================
def run_against_tap(gen, n, steps, top_n, what, codes=None):
    cfg = gen.lm_model.config
    codes = codes or user_codes(cfg, n, steps, gen.device)
    with gen.streaming(n):
        for s in range(steps):
            _, tl, al = gen.step_with_taps(codes[s])
            assert tl.shape[0] == n
            assert_last_is_tap(gen, tl, al, range(n), top_n, f"{what} step {s}")


def check_guided(device, lib, no_text: bool, n=2, steps=3, top_n=2):
    cfg, lm = tiny_model(device, lib, 2 * n, fuser=ConditionFuser({"sum": ["c"]}))
    g = torch.Generator().manual_seed(3)
    cs = (0.5 * torch.randn(2 * n, 1, cfg.dim, generator=g)).to(torch.bfloat16)
    gen = LMGen(lm, use_sampling=True, seed=4, support_out_of_sync=True, cfg_coef=2.0, cfg_is_no_text=no_text, logprobs=top_n,
                condition_tensors={"c": (cs, torch.ones(2 * n, 1, dtype=torch.bool))})
    run_against_tap(gen, n, steps, top_n, f"guided (no_text={no_text})")


def check_other_handle(device, lib, kind: str, steps=2, top_n=2):
    n, cfg, kw = 2, None, {}
    if kind == "int8":
        kw = dict(quantize=True)
    elif kind == "kv_fp4":
        kw = dict(kv_cache="fp4")
    elif kind == "rows96":
        n, kw = 70, dict(max_rows=96)
    elif kind == "stt":
        cfg = tiny_stt_config()
    else:
        raise AssertionError(kind)
    cfg, lm = tiny_model(device, lib, n, cfg, **kw)
    run_against_tap(LMGen(lm, use_sampling=True, seed=6, support_out_of_sync=True, logprobs=top_n), n, steps, top_n, kind)


def check_tts_machine(device, lib, steps=3, top_n=2):
    from tests import tts_machine_cases as tm
    g = tm.golden("lm_tts_machine.npz")
    gen = tm.tts_gen(device, lib, tm.lm_machine(g), logprobs=top_n)
    gen.streaming_forever(3)
    try:
        for b, sc in tm.lm_scripts(g).items():
            gen.set_session_script(b, sc)
        for s in range(steps):
            _, tl, al = gen.step_with_taps(tm.codes_for(gen, 3))
            assert_last_is_tap(gen, tl, al, range(3), top_n, f"TTS machine step {s}")
    finally:
        gen._stop_streaming()
        _capi_off(gen.lm_model)


def _capi_off(lm):
    """The option belongs to the handle: a cached model shared with other tests goes back to off."""
    lm._lib.check(lm._lib.mmi_lm_enable_logprobs(lm._handle, 0, 0))


# ==== Part E: the off state, and a repeat =================================================================================================
def stream(gen, n, codes, with_lp=False):
    toks, lps, ll, nbytes = [], [], None, 0
    with gen.streaming(n):
        for c in codes:
            out = gen.step(c)
            toks.append(out.cpu().numpy()[:, :, 0])
            if with_lp:
                lps.append(lp_arrays(gen.last_logprobs()) + lp_arrays(gen.frame_logprobs()))
        ll = gen.launch_list()
        nbytes = gen.get_streaming_state()["lm_gen"].numel()
    return np.stack(toks), lps, ll, nbytes


def check_off_state_and_repeat(device, lib, n=3, steps=5, top_n=8):
    cfg, lm_off = tiny_model(device, lib, n)
    _, lm_on = tiny_model(device, lib, n)
    codes = user_codes(cfg, n, steps, device)
    kw = dict(use_sampling=True, temp=0.9, temp_text=0.8, seed=11, support_out_of_sync=True)
    t_off, _, ll_off, b_off = stream(LMGen(lm_off, **kw), n, codes)
    t_on, lp_on, ll_on, b_on = stream(LMGen(lm_on, logprobs=top_n, **kw), n, codes, True)
    assert (t_off >= 0).any() and np.array_equal(t_off, t_on), "the enabled handle samples other tokens"
    assert b_off == b_on, "the streaming state changed size"
    at = [i for i, (site, _) in enumerate(ll_on) if site == "logprob"]
    assert len(at) == 1 and ll_on[at[0]] == ("logprob", "k_step_logprob") and ll_on[at[0] + 1][0] == "commit"
    assert ll_on[:at[0]] + ll_on[at[0] + 1:] == ll_off, "the enabled launch list is not the plain one plus one op"
    assert not any("logprob" in k or "k_lp_" in k for _, k in ll_off)
    with LMGen(lm_off, **kw).streaming(n):                        # a plain handle has nothing to read
        assert lm_off._lib.mmi_lm_logprobs_enabled(lm_off._handle, None) == 0
    t_again, lp_again, _, _ = stream(LMGen(lm_on, logprobs=top_n, **kw), n, codes, True)
    assert np.array_equal(t_on, t_again)
    assert all(same_bits(a, b) for x, y in zip(lp_on, lp_again) for a, b in zip(x, y)), "a repeated stream gave other log-probability bytes"
    # the same handle with the option off again is the plain handle
    t_back, _, ll_back, _ = stream(LMGen(lm_on, **kw), n, codes)
    assert np.array_equal(t_back, t_off) and ll_back == ll_off


# ==== Part F: the batcher =================================================================================================================
def check_batcher(device, lib, top_n=2):
    """batcher_cases.check_batcher_matches_manual_api's recipe with the option on: the batcher's frames and their log-probabilities
    against the same schedule by hand (`frame_logprobs()` behind every hand-driven step)."""
    slots = 3
    mimi_a, lm_a, mcfg, lcfg = bc.tiny_pair(device, lib, slots)
    mimi_b, lm_b, _, _ = bc.tiny_pair(device, lib, slots)
    mimi_c, lm_c, _, _ = bc.tiny_pair(device, lib, slots)
    with SessionBatcher(mimi_c, lm_c, slots, use_sampling=False) as plain:
        res_plain, _ = bc.scripted_run(plain, None, mcfg.frame_size)
        with pytest.raises(RuntimeError):                         # MMI_ERR_STATE: the handle did not enable the option
            plain.pop_with_logprobs(plain.open())
    manual = bc.ManualLoop(mimi_b, lm_b, slots, logprobs=top_n)
    F = mcfg.frame_size
    rng, live, slot_of, fed, chan, res, ref = {}, [], {}, {}, {}, {}, {}
    reopened = False
    with SessionBatcher(mimi_a, lm_a, slots, use_sampling=False, logprobs=top_n) as batcher:
        for step in range(bc.N_STEPS):
            acts = [(a, s) for (t, a, s) in bc.SCRIPT if t == step]
            resets, skips = set(), set()
            for a, s in acts:
                if a == "open":
                    chan[s] = batcher.open()
                    used = set(slot_of.values())
                    slot_of[s] = min(r for r in range(slots) if r not in used)
                    live.append(s)
                    fed[s] = 0
                    rng[s] = np.random.default_rng(sum(map(ord, s)))
                    res[s], ref[s] = [], []
                    resets.add(slot_of[s])
                elif a == "close":
                    batcher.close(chan[s])
                    live.remove(s)
                    del slot_of[s]
                else:
                    skips.add(s)
            frames, firsts = {}, set()
            for s in live:
                if s in skips:
                    continue
                x = (0.3 * rng[s].standard_normal(F)).astype(np.float32)
                cut = int(rng[s].integers(1, F))                  # (scripted_run's draws: the plain batcher above gets the same audio)
                batcher.push(chan[s], x[:cut])
                batcher.push(chan[s], x[cut:])
                frames[slot_of[s]] = x
                if fed[s] == 0:
                    firsts.add(slot_of[s])
                fed[s] += 1
            assert batcher.step() == len(frames)
            got = manual.step(frames, resets, firsts)
            fl = lp_arrays(manual.gen.frame_logprobs())
            # the batcher's LM, read directly: a slot reopened by a new channel starts from NaN
            mine = lp_arrays(_read(lm_a, slots, top_n, frame=True))
            for r in resets:
                assert_nothing_recorded(tuple(m[r] for m in mine), Ellipsis, f"step {step}: reopened slot {r}")
                reopened = reopened or step > 0
            for s in live:
                if slot_of[s] in got:
                    ref[s].append(got[slot_of[s]] + tuple(f[slot_of[s]] for f in fl))
                while True:                                       # `pop` next to `pop_with_logprobs`: every other frame of y without them
                    f = batcher.pop(chan[s]) if s == "y" and len(res[s]) % 2 else batcher.pop_with_logprobs(chan[s])
                    if f is None:
                        break
                    res[s].append(f)
    manual.stop()
    assert reopened
    played = 0
    for s in res:
        assert len(res[s]) == len(ref[s]) == len(res_plain[s]), f"session {s}: frame counts differ"
        for i, (a, b, p) in enumerate(zip(res[s], ref[s], res_plain[s])):
            assert np.array_equal(a[1], p[1]) and np.array_equal(a[0], p[0]), f"session {s} frame {i}: the option changed the frame"
            assert np.array_equal(a[1], b[1]), f"session {s} frame {i}: tokens differ from the hand-driven schedule"
            if len(a) > 2:
                assert all(same_bits(x, y) for x, y in zip(a[2:], b[2:])), f"session {s} frame {i}: log-probabilities differ"
                assert np.isfinite(a[2]).all() and (a[3] >= 0).all()
                played += 1
    assert played > 8


def _read(lm, B, top_n, frame):
    from moshi_amd.lm import LogProbs
    S = 1 + lm.dep_q
    logp = torch.empty(B, S, dtype=torch.float32, device=lm.device)
    ids = torch.empty(B, S, top_n, dtype=torch.int32, device=lm.device)
    tlp = torch.empty(B, S, top_n, dtype=torch.float32, device=lm.device)
    fn = lm._lib.mmi_lm_frame_logprobs if frame else lm._lib.mmi_lm_last_logprobs
    lm._lib.check(fn(lm._handle, logp.data_ptr(), ids.data_ptr() if top_n else None, tlp.data_ptr() if top_n else None,
                     _capi.stream_ptr(lm.device)))
    return LogProbs(logp, ids.to(torch.int64), tlp)


# ==== Part G: refusals ====================================================================================================================
def check_refusals(device, lib, n=2):
    cfg, lm = tiny_model(device, lib, n)
    L, h = lm._lib, lm._handle
    codes = user_codes(cfg, n, 2, device)
    S = 1 + cfg.dep_q
    logp = torch.empty(n, S, dtype=torch.float32, device=lm.device)
    ids = torch.empty(n, S, 8, dtype=torch.int32, device=lm.device)
    tlp = torch.empty(n, S, 8, dtype=torch.float32, device=lm.device)
    st = _capi.stream_ptr(lm.device)
    for bad in (-1, 9):
        assert L.mmi_lm_enable_logprobs(h, 1, bad) == _capi.MMI_ERR_INVALID
        with pytest.raises(ValueError):
            LMGen(lm, logprobs=bad).streaming_forever(n)
    top = C.c_int32(-5)
    assert L.mmi_lm_logprobs_enabled(h, C.byref(top)) == 0 and top.value == 0
    # not enabled / not streaming
    assert L.mmi_lm_last_logprobs(h, logp.data_ptr(), None, None, st) == _capi.MMI_ERR_STATE
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    with gen.streaming(n):
        gen.step(codes[0])
        for fn in (L.mmi_lm_last_logprobs, L.mmi_lm_frame_logprobs):
            assert fn(h, logp.data_ptr(), None, None, st) == _capi.MMI_ERR_STATE
        with pytest.raises(RuntimeError):
            gen.last_logprobs()
        assert L.mmi_lm_enable_logprobs(h, 1, 2) == _capi.MMI_ERR_STATE         # enabling while streaming
        gen.step(codes[1])                                                          # the stream goes on
    assert L.mmi_lm_enable_logprobs(h, 1, 0) == 0
    assert L.mmi_lm_logprobs_enabled(h, C.byref(top)) == 1 and top.value == 0
    assert L.mmi_lm_frame_logprobs(h, logp.data_ptr(), None, None, st) == _capi.MMI_ERR_STATE   # enabled, not streaming
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, logprobs=0)
    with gen.streaming(n):
        gen.step(codes[0])
        for fn in (L.mmi_lm_last_logprobs, L.mmi_lm_frame_logprobs):
            assert fn(h, None, None, None, st) == _capi.MMI_ERR_INVALID            # a null logp
            assert fn(h, logp.data_ptr(), ids.data_ptr(), tlp.data_ptr(), st) == _capi.MMI_ERR_INVALID      # top_* on top_n == 0
        lp = gen.last_logprobs()
        assert np.isfinite(lp.logp.cpu().numpy()).all() and lp.top_ids.shape == (n, S, 0)
    # the tap
    row = torch.zeros(1, 40, dtype=torch.bfloat16, device=lm.device)
    tg = torch.zeros(1, dtype=torch.int32, device=lm.device)
    for bad_n in (12, 32776):
        assert L.mmi_lm_debug_step_logprob(h, row.data_ptr(), tg.data_ptr(), 1, bad_n, 0, logp.data_ptr(), None, None, st) == _capi.MMI_ERR_UNSUPPORTED
    assert L.mmi_lm_debug_step_logprob(h, row.data_ptr() + 2, tg.data_ptr(), 1, 8, 0, logp.data_ptr(), None, None, st) == _capi.MMI_ERR_UNSUPPORTED
    assert L.mmi_lm_debug_step_logprob(h, row.data_ptr(), tg.data_ptr(), 1, 8, 9, logp.data_ptr(), None, None, st) == _capi.MMI_ERR_INVALID
    assert L.mmi_lm_debug_step_logprob(h, row.data_ptr(), tg.data_ptr(), 1, 8, 0, None, None, None, st) == _capi.MMI_ERR_INVALID
    assert L.mmi_lm_debug_step_logprob(h, row.data_ptr(), tg.data_ptr(), 1, 8, 0, logp.data_ptr(), ids.data_ptr(), tlp.data_ptr(), st) == _capi.MMI_ERR_INVALID
    with pytest.raises(NotImplementedError):
        lm.debug_step_logprob(torch.zeros(1, 12), torch.zeros(1, dtype=torch.int32), 0)
    # NULL handles: a negative status from every entry
    for rc in (L.mmi_lm_enable_logprobs(None, 1, 0), L.mmi_lm_logprobs_enabled(None, None), L.mmi_lm_last_logprobs(None, None, None, None, None),
               L.mmi_lm_frame_logprobs(None, None, None, None, None), L.mmi_lm_debug_step_logprob(None, None, None, 1, 8, 0, None, None, None, None),
               L.mmi_batcher_pop_logprobs(None, 0, None, None, None, None, None, None)):
        assert rc < 0
    # the handle is usable afterwards
    good = lm.debug_step_logprob(torch.zeros(1, 8), torch.zeros(1, dtype=torch.int32), 1)
    assert abs(float(good.logp[0]) + np.log(8)) <= LOGP_TOL and int(good.top_ids[0, 0]) == 0
    run_against_tap(LMGen(lm, use_sampling=False, support_out_of_sync=True, logprobs=1), n, 2, 1, "after the refusals")
