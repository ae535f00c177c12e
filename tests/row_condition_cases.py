"""Cases for per-session conditions (mmi_lm_set_row_condition, mmi_lm_set_cross_capacity, mmi_batcher_open_cond), shared by the
simulator tests (tests/test_row_condition_sim.py) and the GPU tests (tests/test_b_row_condition_gpu.py).

A session of a live stream gets its own `sum` row, its own cross-attention source of its own length and its own guidance
coefficient.  Two kinds of comparison, no tolerance of their own:
  exact    a session of a mixed stream against the same row of a stream that was STARTED with that session's condition for
           every row (today's path: `cross_len` = the session's length, capacity = that length), tokens and tap logits bit for bit;
  oracle   a session against a one-session `LMOracle` with that session's condition and coefficient, ring outputs identical and
           logits within `lm_cases.logits_close`, widened by `lm_cases.GUIDED_WIDEN` for guided sessions as `check_cfg_scenario`
           does.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import torch

from moshi_amd.config import LMConfig, tiny_lm_config
from moshi_amd.lm import ConditionFuser, LMGen, LMModel, SessionCondition
from oracle.lm_oracle import LMOracle
from tests.lm_cases import GUIDED_WIDEN, cached_lm_state_dict, logits_close

SEED = 57


def tiny_cross_config():
    return replace(tiny_lm_config(), cross_attention=True)          # head dim 32: 16 position slots per pass


def wide_cross_config():
    return replace(LMConfig(num_layers=2, context=64), cross_attention=True)   # head dim 128: 4 position slots per pass


_MODELS: dict = {}


def model(device, lib, cfg, max_batch):
    """One engine per (library, architecture, tile): the weights of the full-width config are a second of upload each."""
    key = (str(device), id(lib), repr(cfg), max_batch)
    if key not in _MODELS:
        while len(_MODELS) >= 2:
            _MODELS.pop(next(iter(_MODELS)))
        _MODELS[key] = LMModel(cached_lm_state_dict(cfg, SEED), cfg, device=device, max_batch=max_batch, lib=lib,
                               fuser=ConditionFuser({"sum": ["s"], "cross": ["x"]}))
    return _MODELS[key]


def session_cond(cfg, tag, length, R):
    """A session's own condition: (sum [R, 1, dim], cross [R, length, dim]) bf16, R model rows (conditioned first)."""
    g = torch.Generator().manual_seed(SEED * 1000 + tag)
    cs = (0.5 * torch.randn(R, 1, cfg.dim, generator=g)).to(torch.bfloat16)
    cx = (0.7 * torch.randn(R, length, cfg.dim, generator=g)).to(torch.bfloat16)
    return cs, cx


def tensors(conds):
    """Condition tensors for LMGen / SessionCondition from a list of session conditions of one length: the conditioned rows of
    every session first, then their unconditioned twins (lm.py:646-651)."""
    R = conds[0][0].shape[0]
    cs = torch.cat([c[0][r:r + 1] for r in range(R) for c in conds])
    cx = torch.cat([c[1][r:r + 1] for r in range(R) for c in conds])
    return {"s": (cs, torch.ones(cs.shape[:2], dtype=torch.bool)), "x": (cx, torch.ones(cx.shape[:2], dtype=torch.bool))}


def user_codes(cfg, B, steps, seed=SEED):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1)) for _ in range(steps)]


def take(gen, codes, device, forced=None):
    f = None if forced is None else torch.from_numpy(forced).to(device)
    out, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device), forced_tokens=f)
    return out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy()


def same_bits(a, b, what):
    for name, x, y in zip(("tokens", "text logits", "audio logits"), a, b):
        assert np.array_equal(x, y) and x.dtype == y.dtype, f"{what}: {name} differ"


def uniform_run(lm, cond, B, codes, device, coef=1.0):
    """Today's path: a stream whose every row is started with `cond` (capacity = its length)."""
    lm.set_cross_capacity(None)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=coef, condition_tensors=tensors([cond] * B))
    with gen.streaming(B):
        return [take(gen, c, device) for c in codes]


def mixed_start(lm, conds, coefs, device, cap=None):
    """A stream started with session 0's condition for everybody, then every session set to its own."""
    B = len(conds)
    guided = any(c != 1.0 for c in coefs)
    lm.set_cross_capacity(cap or max(c[1].shape[1] for c in conds))
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=next(c for c in coefs if c != 1.0) if guided else 1.0,
                condition_tensors=tensors([conds[0]] * B))
    gen.streaming_forever(B)
    for b in range(B):
        gen.set_session_condition(b, SessionCondition(cfg_coef=coefs[b], condition_tensors=tensors([conds[b]])))
    return gen


# ---- 1. mixed lengths equal uniform streams, bit for bit -------------------------------------------------------------------------------
def check_mixed_equals_uniform(device, lib, cfg, lengths, steps, cap=None):
    B = len(lengths)
    lm = model(device, lib, cfg, B)
    conds = [session_cond(cfg, b, L, 1) for b, L in enumerate(lengths)]
    codes = user_codes(cfg, B, steps)
    gen = mixed_start(lm, conds, [1.0] * B, device, cap)
    try:
        mixed = [take(gen, c, device) for c in codes]
    finally:
        gen._stop_streaming()
    for b, L in enumerate(lengths):
        # sessions that share a length still have their own source: every one gets its own uniform stream
        ref = uniform_run(lm, conds[b], B, codes, device)
        for s in range(steps):
            same_bits([x[b] for x in mixed[s]], [x[b] for x in ref[s]], f"session {b} (length {L}) step {s}")
    assert any(not np.array_equal(mixed[-1][1][0], mixed[-1][1][b]) for b in range(1, B)), "the conditions change nothing: nothing shown"


# ---- 2. each session against a one-session oracle ---------------------------------------------------------------------------------------
def oracle_for(sd, cfg, cond, coef):
    orc = LMOracle(sd, cfg)
    R = 2 if coef != 1.0 else 1
    orc.streaming(1, cfg_coef=coef, condition_sum=cond[0][:R, 0].float().numpy(), condition_cross=cond[1][:R].float().numpy())
    return orc


def check_sessions_vs_oracle(device, lib, cfg, coefs, lengths, steps):
    B = len(coefs)
    lm = model(device, lib, cfg, 2 * B)
    sd = cached_lm_state_dict(cfg, SEED)
    conds = [session_cond(cfg, 10 + b, L, 2) for b, L in enumerate(lengths)]
    orcs = [oracle_for(sd, cfg, conds[b], coefs[b]) for b in range(B)]
    codes = user_codes(cfg, B, steps)
    gen = mixed_start(lm, conds, coefs, device)
    try:
        for s in range(steps):
            o = [orcs[b].step(codes[s][b:b + 1], use_sampling=False, support_out_of_sync=True) for b in range(B)]
            forced = np.stack([np.concatenate([o[b][1][2][:1], o[b][1][3][0]]) for b in range(B)])
            out, tl, al = take(gen, codes[s], device, forced)
            for b in range(B):
                oo, (otl, oal, _, _) = o[b]
                wd = GUIDED_WIDEN if coefs[b] != 1.0 else 1.0
                assert np.array_equal(out[b], oo[0]), f"step {s} session {b}: ring output differs"
                print(f"step {s} session {b} coef {coefs[b]}: text max|d| {np.abs(tl[b] - otl[0]).max():.4f} of {np.abs(otl[0]).max():.3f}")
                assert logits_close(tl[b], otl[0], wd), f"step {s} session {b}: text logits"
                for k in range(cfg.dep_q):
                    assert logits_close(al[b, k], oal[0, k], wd), f"step {s} session {b} cb {k}: audio logits"
    finally:
        gen._stop_streaming()


# ---- 3. a change mid-stream touches one session -----------------------------------------------------------------------------------------
def check_change_mid_stream(device, lib, cfg=None, lengths=(5, 17, 3, 16), new_length=20, before=3, after=3):
    cfg = cfg or tiny_cross_config()
    B = len(lengths)
    lm = model(device, lib, cfg, 2 * B)
    coefs = [2.0, 1.0, 0.5, 3.0][:B]
    conds = [session_cond(cfg, 20 + b, L, 2) for b, L in enumerate(lengths)]
    new = session_cond(cfg, 29, new_length, 2)
    codes = user_codes(cfg, B, before + after)
    cap = max(max(lengths), new_length)
    lib_ = lm._lib

    def run(change):
        gen = mixed_start(lm, conds, coefs, device, cap)
        res = []
        try:
            for s, c in enumerate(codes):
                if change and s == before:
                    captured = int(lib_.mmi_lm_stat(lm._handle, 1))
                    gen.set_session_condition(1, SessionCondition(cfg_coef=1.5, condition_tensors=tensors([new])))
                    m = torch.zeros(B, dtype=torch.bool); m[1] = True
                    gen.reset_streaming(m.to(device))
                    assert int(lib_.mmi_lm_stat(lm._handle, 1)) == captured, "a condition change captured a step program"
                res.append(take(gen, c, device))
                if change and s == before:
                    assert int(lib_.mmi_lm_stat(lm._handle, 1)) == captured, "the step after a condition change captured a program"
        finally:
            gen._stop_streaming()
        return res
    plain, changed = run(False), run(True)
    for s in range(before + after):
        for b in range(B):
            if b != 1 or s < before:
                same_bits([x[b] for x in changed[s]], [x[b] for x in plain[s]], f"session {b} step {s}: touched by session 1's change")
    # session 1 from the change on: row 1 of a fresh guided stream started with the new condition for every row
    ref = uniform_run(lm, new, B, codes[before:], device, coef=1.5)
    for s in range(after):
        same_bits([x[1] for x in changed[before + s]], [x[1] for x in ref[s]], f"session 1, step {s} after its change")
    assert not np.array_equal(changed[before][1][1], plain[before][1][1]), "the new condition changes nothing: nothing shown"


# ---- 4. snapshot ----------------------------------------------------------------------------------------------------------------------
def check_snapshot(device, lib, lengths=(3, 17, 9), steps=4):
    cfg = tiny_cross_config()
    B = len(lengths)
    lm = model(device, lib, cfg, 2 * B)
    conds = [session_cond(cfg, 30 + b, L, 1) for b, L in enumerate(lengths)]
    other = session_cond(cfg, 39, 12, 1)
    codes = user_codes(cfg, B, steps)

    def run(interrupt):
        gen = mixed_start(lm, conds, [1.0] * B, device, 20)
        res = []
        try:
            nbytes = int(lm._lib.mmi_lm_state_bytes(lm._handle))
            for s, c in enumerate(codes):
                if interrupt and s == 2:
                    snap = gen.get_streaming_state()
                    gen.set_session_condition(0, SessionCondition(condition_tensors=tensors([other])))
                    take(gen, c, device)
                    gen.set_streaming_state(snap)
                res.append(take(gen, c, device))
        finally:
            gen._stop_streaming()
        return res, nbytes
    (a, n20), (b, _) = run(False), run(True)
    for s in range(steps):
        same_bits(a[s], b[s], f"step {s} after save / change / load")
    gen = mixed_start(lm, conds, [1.0] * B, device, 40)
    n40 = int(lm._lib.mmi_lm_state_bytes(lm._handle))
    gen._stop_streaming()
    assert n40 - n20 >= cfg.num_layers * B * 20 * 2 * cfg.dim * 2, (n20, n40)     # 20 more positions of bf16 keys | values per row and layer


# ---- 5. repeat streams ----------------------------------------------------------------------------------------------------------------
GUIDED_COEFS = [2.0, 1.0, 0.5, 3.0]
GUIDED_LENGTHS = [1, 16, 17, 7]


def guided_mixed_run(device, lib, cfg, B, steps):
    lm = model(device, lib, cfg, 2 * B)
    coefs = [GUIDED_COEFS[b % 4] for b in range(B)]
    conds = [session_cond(cfg, 10 + b, GUIDED_LENGTHS[b % 4], 2) for b in range(B)]
    gen = mixed_start(lm, conds, coefs, device)
    try:
        return [take(gen, c, device) for c in user_codes(cfg, B, steps)]
    finally:
        gen._stop_streaming()


def check_repeat_streams(device, lib, cfg=None, B=4, steps=3, runs=3):
    cfg = cfg or tiny_cross_config()
    first = guided_mixed_run(device, lib, cfg, B, steps)
    for r in range(1, runs):
        again = guided_mixed_run(device, lib, cfg, B, steps)
        for s in range(steps):
            same_bits(first[s], again[s], f"run {r} step {s}")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def check_refusals(device, lib):
    import ctypes as C
    import pytest
    from moshi_amd import _capi
    cfg = tiny_cross_config()
    B = 2
    lm = model(device, lib, cfg, 2 * B)
    lib_ = lm._lib
    conds = [session_cond(cfg, 40 + b, 5, 2) for b in range(B)]
    one = [(c[0][:1], c[1][:1]) for c in conds]
    codes = user_codes(cfg, B, 3)
    good = SessionCondition(condition_tensors=tensors([one[0]]))
    lm.set_cross_capacity(None)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, condition_tensors=tensors(one))
    with pytest.raises(AssertionError):
        gen.set_session_condition(0, good)                                              # not streaming (the Python guard)
    rc = _capi.RowCondition()
    rc.cfg_coef = 1.0
    with pytest.raises(RuntimeError):
        lib_.check(lib_.mmi_lm_set_row_condition(lm._handle, 0, C.byref(rc), None))     # MMI_ERR_STATE

    def ref_run(g):
        with g.streaming(B):
            return [take(g, c, device) for c in codes]
    want = ref_run(gen)
    with gen.streaming(B):
        got = [take(gen, codes[0], device)]
        for session in (-1, B):
            with pytest.raises(ValueError):
                gen.set_session_condition(session, good)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError):
                gen.set_session_condition(0, SessionCondition(cfg_coef=bad))
        with pytest.raises(RuntimeError):
            gen.set_session_condition(0, SessionCondition(cfg_coef=2.0))                # the stream has no twin rows
        for L in (0, 6):                                                                # capacity = the start's 5 positions
            x = _capi.RowCondition()
            x.cfg_coef, x.cross_len = 1.0, L
            keep = torch.zeros(1, 6, cfg.dim, dtype=torch.bfloat16, device=device)
            x.condition_cross = keep.data_ptr()
            with pytest.raises(AssertionError):
                lib_.check(lib_.mmi_lm_set_row_condition(lm._handle, 0, C.byref(x), gen._stream()))
        with pytest.raises(RuntimeError):
            lm.set_cross_capacity(8)                                                    # not while streaming
        got += [take(gen, c, device) for c in codes[1:]]
    for s in range(3):
        same_bits(want[s], got[s], f"step {s} after the refusals")
    # a stream without a sum condition has no buffer for one
    lm_nosum = LMModel(cached_lm_state_dict(cfg, SEED), cfg, device=device, max_batch=B, lib=lib, fuser=ConditionFuser({"sum": [], "cross": ["x"]}))
    gen2 = LMGen(lm_nosum, use_sampling=False, support_out_of_sync=True, condition_tensors={"x": tensors(one)["x"]})
    with gen2.streaming(B):
        a = take(gen2, codes[0], device)
        x = _capi.RowCondition()
        x.cfg_coef = 1.0
        keep = torch.zeros(1, cfg.dim, dtype=torch.bfloat16, device=device)
        x.condition_sum = keep.data_ptr()
        with pytest.raises(RuntimeError):
            lib_.check(lib_.mmi_lm_set_row_condition(lm_nosum._handle, 0, C.byref(x), gen2._stream()))
    with gen2.streaming(B):
        same_bits(a, take(gen2, codes[0], device), "the handle after a refused sum condition")
    # a model without cross-attention layers
    plain_cfg = tiny_lm_config()
    lm_plain = LMModel(cached_lm_state_dict(plain_cfg, SEED), plain_cfg, device=device, max_batch=B, lib=lib)
    gen3 = LMGen(lm_plain, use_sampling=False, support_out_of_sync=True)
    with gen3.streaming(B):
        x = _capi.RowCondition()
        x.cfg_coef, x.cross_len = 1.0, 1
        keep = torch.zeros(1, 1, plain_cfg.dim, dtype=torch.bfloat16, device=device)
        x.condition_cross = keep.data_ptr()
        with pytest.raises(ValueError):
            lib_.check(lib_.mmi_lm_set_row_condition(lm_plain._handle, 0, C.byref(x), gen3._stream()))
        take(gen3, codes[0], device)
    # a capacity below the start's cross_len is refused at start, and the handle starts again afterwards
    lm.set_cross_capacity(4)
    with pytest.raises(AssertionError):
        gen.streaming_forever(B)
    lm.set_cross_capacity(None)
    same_bits(want[0], ref_run(gen)[0], "the handle after a refused start")


# ---- 7. the batcher -------------------------------------------------------------------------------------------------------------------
def check_batcher_conditions(device, lib, n=8):
    """Channels a, b, c open at steps 0, 2, 4 with conditions of their own (a: coefficient only); a closes at step 3, so c takes
    slot 0 - a slot whose last owner had a condition - with another one; b closes at step 5 and d opens at step 6 into b's slot
    WITHOUT a condition: it must run on the batcher's own cfg.guidance rows again.  Every frame equals the same schedule driven
    by hand through MimiModel / LMGen.set_session_condition."""
    import pytest
    from moshi_amd.batcher import SessionBatcher
    from moshi_amd.config import tiny_mimi_config
    from moshi_amd.mimi import MimiModel
    from moshi_amd.weights import random_mimi_state_dict
    from tests.batcher_cases import ManualLoop
    slots = 2
    cfg = tiny_cross_config()
    mcfg = replace(tiny_mimi_config(), q_bins=cfg.card, q_n_q=cfg.dep_q)
    msd = random_mimi_state_dict(mcfg, seed=5)
    fuser = ConditionFuser({"sum": ["s"], "cross": ["x"]})

    def pair():
        return (MimiModel(msd, mcfg, device=device, max_batch=slots, num_codebooks=cfg.dep_q, lib=lib),
                LMModel(cached_lm_state_dict(cfg, SEED), cfg, device=device, max_batch=2 * slots, lib=lib, fuser=fuser, cross_capacity=18))
    base = tensors([session_cond(cfg, 50 + r, 6, 2) for r in range(slots)])
    own = {"a": SessionCondition(cfg_coef=1.0), "b": SessionCondition(cfg_coef=0.5, condition_tensors=tensors([session_cond(cfg, 61, 17, 2)])),
           "c": SessionCondition(cfg_coef=3.0, condition_tensors=tensors([session_cond(cfg, 62, 1, 2)])), "d": None}
    script = {0: [("open", "a", 0)], 2: [("open", "b", 1)], 3: [("close", "a", 0)], 4: [("open", "c", 0)], 5: [("close", "b", 1)],
              6: [("open", "d", 1)]}
    F = mcfg.frame_size
    pcm = {c: (0.3 * np.random.default_rng(ord(c)).standard_normal((n, F))).astype(np.float32) for c in own}
    (mimi_a, lm_a), (mimi_b, lm_b) = pair(), pair()
    manual = ManualLoop(mimi_b, lm_b, slots, cfg_coef=2.0, condition_tensors=base)
    res, ref = {c: [] for c in own}, {c: [] for c in own}
    had_cond = [False] * slots
    try:
        with SessionBatcher(mimi_a, lm_a, slots, use_sampling=False, cfg_coef=2.0, condition_tensors=base) as b:
            with pytest.raises(AssertionError):                                         # longer than the handle's capacity: no slot claimed
                b.open(condition=SessionCondition(cfg_coef=2.0, condition_tensors=tensors([session_cond(cfg, 63, 19, 2)])))
            with pytest.raises(ValueError):
                b.open(condition=SessionCondition(cfg_coef=float("nan")))
            assert b.used_slots == 0
            chan, slot, fed = {}, {}, {}
            for t in range(n):
                resets = set()
                for act, c, r in script.get(t, []):
                    if act == "open":
                        chan[c] = b.open(condition=own[c])
                        slot[c], fed[c] = r, 0
                        resets.add(r)
                        if own[c] is not None:
                            manual.gen.set_session_condition(r, own[c])
                        elif had_cond[r]:       # by hand: the slot's rows of the batcher's own condition again
                            manual.gen.set_session_condition(r, SessionCondition(cfg_coef=2.0, condition_tensors={
                                k: (v[0][[r, slots + r]], v[1][[r, slots + r]]) for k, v in base.items()}))
                        had_cond[r] = own[c] is not None
                    else:
                        b.close(chan.pop(c))
                        del slot[c]
                frames, firsts = {}, set()
                for c, r in slot.items():
                    b.push(chan[c], pcm[c][fed[c]])
                    frames[r] = pcm[c][fed[c]]
                    if fed[c] == 0:
                        firsts.add(r)
                    fed[c] += 1
                assert b.step() == len(frames)
                got = manual.step(frames, resets, firsts)
                for c, r in slot.items():
                    while (fr := b.pop(chan[c])) is not None:
                        res[c].append(fr)
                    if r in got:
                        ref[c].append(got[r])
    finally:
        manual.stop()
    for c in own:
        assert len(res[c]) == len(ref[c]) and len(res[c]) >= 1, (c, len(res[c]), len(ref[c]))
        for i, ((pa, ta), (pb, tb)) in enumerate(zip(res[c], ref[c])):
            assert np.array_equal(ta, tb), f"channel {c} frame {i}: tokens differ from the hand-driven schedule"
            assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), f"channel {c} frame {i}: PCM differs"
    # d against a batcher in which nobody ever had a condition: the same slot, the same frames, the batcher's own rows
    mimi_c, lm_c = pair()
    plain = []
    with SessionBatcher(mimi_c, lm_c, slots, use_sampling=False, cfg_coef=2.0, condition_tensors=base) as b:
        first = b.open()
        ch = b.open()
        b.close(first)
        for t in range(n - 6):
            b.push(ch, pcm["d"][t])
            b.step()
            while (fr := b.pop(ch)) is not None:
                plain.append(fr)
    assert len(plain) == len(res["d"])
    for i, ((pa, ta), (pb, tb)) in enumerate(zip(res["d"], plain)):
        assert np.array_equal(ta, tb), f"frame {i}: a slot reopened without a condition is not back on cfg.guidance"


# ---- 8. layout ------------------------------------------------------------------------------------------------------------------------
def check_layout(tmp_path, root):
    import ctypes
    import subprocess
    from moshi_amd import _capi
    for cname, cls in (("mmi_row_condition", _capi.RowCondition), ("mmi_batcher_condition", _capi.BatcherCondition)):
        fields = [n for n, _ in cls._fields_]
        assert fields == ["cfg_coef", "condition_sum", "condition_cross", "cross_len"]
        lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "moshi_mi.h"', 'int main(void) {',
                 f'  printf(". %zu\\n", sizeof({cname}));']
        lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f in fields] + ['  return 0;', '}']
        src = tmp_path / f"{cname}.c"
        src.write_text("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-std=c99", f"-I{root / 'include'}", str(src), "-o", str(tmp_path / cname)])
        for ln in subprocess.run([str(tmp_path / cname)], capture_output=True, text=True, check=True).stdout.splitlines():
            f, v = ln.split()
            if f == ".":
                assert ctypes.sizeof(cls) == int(v)
            else:
                assert getattr(cls, f).offset == int(v), f
