"""Cases for forking a live session into other slots (mmi_lm_fork_session, mmi_mimi_fork_session, mmi_batcher_fork; DESIGN.md
8.24), shared by the simulator suite (tests/test_fork_sim.py) and the MI355X suite (tests/test_b_fork_gpu.py).

Every gate is exact.  A session's bits do not depend on its slot (the row-sampling, many-rows and batcher cases hold that), so a
forked session must continue like its source bit for bit, and like a control handle on which the destination slot itself ran the
source's whole history.  The shapes are the tiny models': a temporal ring of 12 positions, 4 heads of 32, 2 layers; a codec ring
of 6 - the source depths cover an empty ring, a partial one, an exactly full one and a wrapped one."""
from __future__ import annotations

import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch

from moshi_amd import _capi
from moshi_amd.config import tiny_lm_config, tiny_mimi_config
from moshi_amd.errors import UnknownChannel
from moshi_amd.lm import ConditionFuser, LMGen, LMModel, SessionCondition, SessionSampling, TTSScript
from moshi_amd.mimi import MimiModel
from moshi_amd.weights import random_mimi_state_dict
from tests import kv4_cases as kc
from tests.lm_cases import cached_lm_state_dict

SEED = 83
PRE = 4             # steps the other sessions run before the source starts: the destination's old state is deeper than the source's
AFTER = 6
DEPTHS = (0, 5, 12, 17)         # of the source at the fork: fresh, partial ring, exactly full, wrapped (context 12)


def ring_config(kv):
    return kc.kv4_config() if kv == "fp4" else replace(tiny_lm_config(), kv_cache_dtype=kv)


def lm_of(device, lib, cfg, **size):
    return LMModel(cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), SEED), cfg, device=device, lib=lib, **size)


def take(gen, codes, device):
    out, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device))
    return out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy()


def same(a, b, ra, rb, what):
    """Tokens, text logits and audio logits of row ra of step result a equal row rb of b, in bits."""
    for name, x, y in zip(("tokens", "text logits", "audio logits"), a, b):
        assert x.dtype == y.dtype and np.array_equal(x[ra].view(np.uint8), y[rb].view(np.uint8)), f"{what}: {name} differ"


def mask_of(B, off, device):
    m = torch.ones(B, dtype=torch.bool)
    for b in off:
        m[b] = False
    return m.to(device)


def codes_of(cfg, B, steps, seed, twins=()):
    """User codes per step; twins: (a, b) pairs - session b gets session a's."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        c = rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))
        for a, b in twins:
            c[b] = c[a]
        out.append(c)
    return out


def ring_planes(gen, B):
    """Every plane of the temporal ring as [rows, H, cap, bytes per position] uint8, keyed by (layer, which, plane)."""
    cfg = gen.lm_model.config
    H, Dh, cap = cfg.num_heads, cfg.dim // cfg.num_heads, cfg.context
    out = {}
    for l in range(cfg.num_layers):
        for which in ("k", "v"):
            raw = gen.kv_ring(l, which).cpu().numpy()
            if cfg.kv_cache_dtype == "fp4":
                c4, s4 = kc.split_planes(raw, B, cfg)
                out[(l, which, "codes")], out[(l, which, "scales")] = c4.copy(), s4.copy()
            else:
                out[(l, which, "values")] = raw.reshape(B, H, cap, -1).copy()
    return out


def check_regions_outside(gen, before, after, touched_rows, what):
    """Every kind-1 region of the snapshot is unchanged outside the slices of `touched_rows` (model rows)."""
    checked = 0
    for name, (off, nbytes, rows, kind) in gen.state_regions().items():
        if kind != 1:
            continue
        a, b = before[off:off + nbytes], after[off:off + nbytes]
        if rows <= 0:
            assert np.array_equal(a, b), f"{what}: region {name} (no per-session slices) changed"
            continue
        a, b = a.reshape(rows, -1), b.reshape(rows, -1)
        keep = [r for r in range(rows) if r not in touched_rows]
        assert np.array_equal(a[keep], b[keep]), f"{what}: region {name} changed outside the destination's slices"
        checked += 1
    assert checked >= 5


# ---- 1. + 2. continuation bit for bit, neighbours untouched ----------------------------------------------------------------------------
def check_continuation(device, lib, kv, d, seeded=False):
    """Batch 4, fork 1 -> 3 with the source `d` steps deep and the destination PRE + d steps deep on other inputs."""
    cfg = ring_config(kv)
    B, cap = 4, cfg.context
    lm = lm_of(device, lib, cfg, max_batch=B)
    mine = SessionSampling(temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=4242)
    pre = codes_of(cfg, B, PRE, SEED + 1)
    hist, hist_c = codes_of(cfg, B, d, SEED + 2), codes_of(cfg, B, d, SEED + 2, twins=[(1, 3)])
    after = codes_of(cfg, B, AFTER, SEED + 3, twins=[(1, 3)])

    def run(kind):
        """fork: the handle under test; plain: the same without the fork; control: slot 3 runs session 1's whole history itself."""
        gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
        res, extra = [], {}
        with gen.streaming(B):
            if seeded:
                gen.set_session_sampling(mine, mask=[0, 1, 0, kind == "control"])
            gen.set_exec_mask(mask_of(B, (1, 3) if kind == "control" else (1,), device))
            for c in pre:
                take(gen, c, device)
            gen.set_exec_mask(mask_of(B, (), device))
            for c in (hist_c if kind == "control" else hist):
                take(gen, c, device)
            if kind == "fork":
                planes0, snap0 = ring_planes(gen, B), gen.get_streaming_state()["lm_gen"].cpu().numpy()
                launches0, bytes0 = gen.launch_list(), int(gen._lib.mmi_lm_state_bytes(lm._handle))
                gen.fork_session(1, 3)
                extra = dict(planes0=planes0, planes1=ring_planes(gen, B), snap0=snap0,
                             snap1=gen.get_streaming_state()["lm_gen"].cpu().numpy())
                check_regions_outside(gen, snap0, extra["snap1"], {3}, f"{kv} d={d}")
                assert bytes0 == int(gen._lib.mmi_lm_state_bytes(lm._handle))
            for c in after:
                res.append(take(gen, c, device))
            if kind == "fork":
                assert gen.launch_list() == launches0 or not launches0, "the fork changed the step's launch list"
        return res, extra
    forked, ex = run("fork")
    plain, _ = run("plain")
    control, _ = run("control")
    for s in range(AFTER):
        same(forked[s], forked[s], 3, 1, f"{kv} d={d} step {s}: the copy against its source")
        same(forked[s], control[s], 1, 1, f"{kv} d={d} step {s}: the source against the control handle")
        same(forked[s], control[s], 3, 3, f"{kv} d={d} step {s}: the copy against the control's slot 3")
        for b in (0, 2):
            same(forked[s], plain[s], b, b, f"{kv} d={d} step {s}: neighbour {b} against the run without the fork")
    assert any(not np.array_equal(forked[s][1][3], plain[s][1][3]) for s in range(AFTER)), "the fork changes nothing: nothing shown"
    # the ring: the source's valid prefix arrived, the destination's positions beyond it and every other row kept their bytes
    valid = min(d, cap)
    for key, p0 in ex["planes0"].items():
        p1 = ex["planes1"][key]
        assert np.array_equal(p1[:3], p0[:3]), f"{key}: a ring row other than the destination changed"
        assert np.array_equal(p1[3][:, :valid], p0[1][:, :valid]), f"{key}: the valid prefix did not arrive"
        assert np.array_equal(p1[3][:, valid:], p0[3][:, valid:]), f"{key}: positions past the source's valid prefix were written"
        if valid < min(PRE + d, cap):
            assert p0[3][:, valid:].any(), f"{key}: the destination held nothing there: nothing shown"


# ---- 3. several destinations ---------------------------------------------------------------------------------------------------------------
def check_several_destinations(device, lib, d=7, steps=5):
    cfg = tiny_lm_config()
    B, dst = 6, (2, 3, 5)
    lm = lm_of(device, lib, cfg, max_batch=B)
    hist = codes_of(cfg, B, d, SEED + 4)
    after = codes_of(cfg, B, steps, SEED + 5, twins=[(0, b) for b in dst])

    def run(seeds):
        gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
        with gen.streaming(B):
            for c in hist:
                take(gen, c, device)
            gen.fork_session(0, dst)
            if seeds:
                sets = [SessionSampling(temp=1.2, temp_text=1.1, top_k=50, top_k_text=25, seed=seeds.get(b, 0)) for b in range(B)]
                gen.set_session_sampling(sets, mask=[b in seeds for b in range(B)])
            return [take(gen, c, device) for c in after]
    greedy = run(None)
    for s in range(steps):
        for b in dst:
            same(greedy[s], greedy[s], b, 0, f"step {s}: destination {b} against the source")
    apart = run({2: 11, 3: 12, 5: 13})
    for s in range(steps):
        same(apart[s], greedy[s], 0, 0, f"step {s}: the source after its copies took seeds of their own")
    path = {b: np.concatenate([np.concatenate([apart[s][0][b].reshape(-1), apart[s][1][b].reshape(-1)]) for s in range(steps)]) for b in dst}
    assert not np.array_equal(path[2], path[3]) and not np.array_equal(path[3], path[5]) and not np.array_equal(path[2], path[5]), \
        "three seeds give the same candidates"


# ---- 4. guided streams -----------------------------------------------------------------------------------------------------------------------
def check_guided(device, lib, cross, d=5, steps=4):
    """Guidance (cfg_coef != 1) with a sum condition; cross: also a cross-attention source of the session's own length.  The source's
    condition is set through set_session_condition; the control gives slot 2 the same condition directly."""
    from tests import row_condition_cases as rcc
    cfg = rcc.tiny_cross_config() if cross else tiny_lm_config()
    B = 3
    fuser = ConditionFuser({"sum": ["s"], "cross": ["x"]} if cross else {"sum": ["s"]})
    lm = LMModel(cached_lm_state_dict(cfg, SEED), cfg, device=device, max_batch=2 * B, lib=lib, fuser=fuser)
    lengths, coefs = (5, 9, 3), (2.0, 1.5, 3.0)
    conds = [rcc.session_cond(cfg, 40 + b, L, 2) for b, L in enumerate(lengths)]

    def tensors(cs):
        t = rcc.tensors(cs)
        return t if cross else {"s": t["s"]}
    hist, hist_c = codes_of(cfg, B, d, SEED + 6), codes_of(cfg, B, d, SEED + 6, twins=[(0, 2)])
    after = codes_of(cfg, B, steps, SEED + 7, twins=[(0, 2)])

    def run(kind):
        mine = [conds[0], conds[1], conds[0] if kind == "control" else conds[2]]
        cf = [coefs[0], coefs[1], coefs[0] if kind == "control" else coefs[2]]
        if cross:
            lm.set_cross_capacity(max(lengths))
        gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=2.0, condition_tensors=tensors([conds[1]] * B))
        with gen.streaming(B):
            for b in range(B):
                gen.set_session_condition(b, SessionCondition(cfg_coef=cf[b], condition_tensors=tensors([mine[b]])))
            for c in (hist_c if kind == "control" else hist):
                take(gen, c, device)
            if kind == "fork":
                snap0 = gen.get_streaming_state()["lm_gen"].cpu().numpy()
                gen.fork_session(0, 2)
                check_regions_outside(gen, snap0, gen.get_streaming_state()["lm_gen"].cpu().numpy(), {2, B + 2}, "guided")
            return [take(gen, c, device) for c in after]
    forked, plain, control = run("fork"), run("plain"), run("control")
    for s in range(steps):
        same(forked[s], forked[s], 2, 0, f"step {s}: the copy against its source")
        same(forked[s], control[s], 2, 2, f"step {s}: the copy against a session given the condition directly")
        same(forked[s], plain[s], 1, 1, f"step {s}: the neighbour")
    assert not np.array_equal(forked[-1][1][2], plain[-1][1][2]), "the fork changes nothing: nothing shown"


def check_guided_after_restore(device, lib, d, steps=3):
    """A guided stream restored from its own snapshot, then forked: mmi_lm_state_load takes the host's ring-depth bound from the
    model rows' offsets, which are one behind the sessions' on a guided stream - the copy must still move the newest ring row.
    d = 1: the bound the load leaves is 0; d = 5: a partial ring.  Distinct conditions per session, so every ring row differs."""
    from tests import row_condition_cases as rcc
    cfg = tiny_lm_config()
    B = 3
    lm = LMModel(cached_lm_state_dict(cfg, SEED), cfg, device=device, max_batch=2 * B, lib=lib, fuser=ConditionFuser({"sum": ["s"]}))
    conds = [rcc.session_cond(cfg, 60 + b, 3, 2) for b in range(B)]
    tensors = lambda cs: {"s": rcc.tensors(cs)["s"]}
    hist = codes_of(cfg, B, d, SEED + 14)
    after = codes_of(cfg, B, steps, SEED + 15, twins=[(0, 2)])

    def run(restore):
        gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=2.0, condition_tensors=tensors(conds))
        with gen.streaming(B):
            for c in hist:
                take(gen, c, device)
            if restore:
                gen.set_streaming_state(gen.get_streaming_state())
            gen.fork_session(0, 2)
            planes = ring_planes(gen, 2 * B)
            return [take(gen, c, device) for c in after], planes
    for restore in (False, True):
        res, planes = run(restore)
        for key, p in planes.items():
            assert p[0][:, :d].any(), f"{key}: the source's ring holds nothing: nothing shown"
            for r in (0, B):
                assert np.array_equal(p[r + 2][:, :d], p[r][:, :d]), f"restore={restore} {key}: model row {r + 2} did not get row {r}'s valid prefix"
        for s in range(steps):
            same(res[s], res[s], 2, 0, f"restore={restore} d={d} step {s}: the copy against its source")
        assert not np.array_equal(res[-1][1][1], res[-1][1][0])


# ---- 5. TTS machine, adapters ------------------------------------------------------------------------------------------------------------------
def check_tts_machine(device, lib, at=6, S=16):
    """The source is mid-script at the fork; the copy finishes the script like the source (tokens and status)."""
    from tests import tts_machine_cases as tm
    g = tm.golden("lm_tts_machine.npz")
    m, scripts = tm.lm_machine(g), tm.lm_scripts(g)
    gen = tm.tts_gen(device, lib, m)
    B = 3
    status = {}

    def ops(s):
        if s == at:
            status["mid"] = gen.session_script_status(0)
            gen.fork_session(0, 2)
    try:
        out, _ = tm.run(gen, B, S, {0: scripts[0], 1: scripts[1], 2: TTSScript(entries=[([33], 0)])}, before_step=ops)
        st = [gen.session_script_status(b) for b in range(B)]
    finally:
        gen._stop_streaming()
    assert 0 < status["mid"].n_consumed < st[0].n_consumed, "the source was not mid-script at the fork: nothing shown"
    assert st[2] == st[0], "the copy's script status differs from the source's"
    assert np.array_equal(out[at:, 2], out[at:, 0]), "the copy's tokens differ from the source's"
    assert not np.array_equal(out[:at, 2], out[:at, 0])


def check_adapter(device, lib, d=4, steps=3):
    from tests import lora_cases as lc
    cfg = tiny_lm_config()
    B = 4
    lm, _ = lc.adapter_model(device, lib, cfg, B, SEED)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    hist = codes_of(cfg, B, d, SEED + 8)
    after = codes_of(cfg, B, steps, SEED + 9, twins=[(1, 3)])
    with gen.streaming(B):
        gen.set_session_adapter(1, 1)
        gen.set_session_adapter(3, 2)
        for c in hist:
            take(gen, c, device)
        gen.fork_session(1, 3)
        assert gen.session_adapter(3) == 1 and gen.session_adapter(1) == 1 and gen.session_adapter(0) is None
        res = [take(gen, c, device) for c in after]
        plain_slot = gen.session_adapter(2)
    assert plain_slot is None
    for s in range(steps):
        same(res[s], res[s], 3, 1, f"step {s}: the copy on the source's adapter slot")


# ---- 6. many rows --------------------------------------------------------------------------------------------------------------------------------
def check_many_rows(device, lib, d=3, steps=3):
    """Batch 96 on a max_rows handle: the copies land in the second 32-row tile and past the 64-row boundary."""
    cfg = tiny_lm_config()
    B, dst = 96, (33, 70)
    lm = lm_of(device, lib, cfg, max_rows=B)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    hist = codes_of(cfg, B, d, SEED + 10)
    after = codes_of(cfg, B, steps, SEED + 11, twins=[(1, b) for b in dst])
    with gen.streaming(B):
        for c in hist:
            take(gen, c, device)
        gen.fork_session(1, dst)
        res = [take(gen, c, device) for c in after]
    for s in range(steps):
        for b in dst:
            same(res[s], res[s], b, 1, f"step {s}: slot {b} against slot 1")
    assert not np.array_equal(res[-1][1][1], res[-1][1][34])


# ---- 7. log-probabilities ----------------------------------------------------------------------------------------------------------------------
def check_logprobs(device, lib, d=5, top_n=2):
    cfg = tiny_lm_config()
    B = 4
    lm = lm_of(device, lib, cfg, max_batch=B)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, logprobs=top_n)
    arrays = lambda lp: (lp.logp.cpu().numpy(), lp.top_ids.cpu().numpy(), lp.top_logp.cpu().numpy())
    with gen.streaming(B):
        for c in codes_of(cfg, B, d, SEED + 12):
            take(gen, c, device)
        before = arrays(gen.last_logprobs())
        assert np.isfinite(before[0][3]).any(), "nothing was recorded for the destination: nothing shown"
        gen.fork_session(1, 3)
        after = arrays(gen.last_logprobs())
        assert np.isnan(after[0][3]).all() and (after[1][3] == -1).all() and np.isnan(after[2][3]).all(), "the destination's rows were not cleared"
        for a, b in zip(before, after):
            assert np.array_equal(a[:3].view(np.uint8), b[:3].view(np.uint8)), "the fork touched another session's log-probabilities"
        c = codes_of(cfg, B, 1, SEED + 13, twins=[(1, 3)])[0]
        take(gen, c, device)
        last = arrays(gen.last_logprobs())
        for x in last:
            assert np.array_equal(x[3].view(np.uint8), x[1].view(np.uint8)), "the copy's next step records other values than the source's"
        assert np.isfinite(last[0][3]).any()


# ---- 8. the codec -----------------------------------------------------------------------------------------------------------------------------
def check_codec(device, lib, f, after=4, pre=2):
    """MimiModel, batch 3: session 0 is `f` frames deep at the fork (ring of 6 positions, 2 per frame), slot 2 pre + f frames."""
    cfg = tiny_mimi_config()
    B, K = 3, cfg.q_n_q
    mimi = MimiModel(random_mimi_state_dict(cfg, seed=SEED), cfg, device=device, max_batch=B, num_codebooks=K, lib=lib)
    F = mimi.frame_size

    def frames(n, seed, twin):
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n):
            pcm = (0.3 * rng.standard_normal((B, 1, F))).astype(np.float32)
            codes = rng.integers(0, cfg.q_bins, (B, K, 1))
            if twin:
                pcm[2], codes[2] = pcm[0], codes[0]
            out.append((pcm, codes))
        return out
    pre_f = frames(pre, SEED + 20, False)
    hist, hist_c = frames(f, SEED + 21, False), frames(f, SEED + 21, True)
    rest = frames(after, SEED + 22, True)

    def one(pcm, codes):
        got = mimi.encode(torch.from_numpy(pcm).to(device)).cpu().numpy()
        return got, mimi.decode(torch.from_numpy(codes).to(device)).cpu().numpy()

    def run(kind):
        with mimi.streaming(B):
            mimi.set_exec_mask(mask_of(B, (0, 2) if kind == "control" else (0,), device))
            for x in pre_f:
                one(*x)
            mimi.set_exec_mask(mask_of(B, (), device))
            for x in (hist_c if kind == "control" else hist):
                one(*x)
            if kind == "fork":
                mimi.fork_session(0, 2)
            return [one(*x) for x in rest]
    forked, plain, control = run("fork"), run("plain"), run("control")
    for s in range(after):
        for i, name in enumerate(("codes", "PCM")):
            bits = lambda r, b: r[s][i][b].view(np.uint8)
            assert np.array_equal(bits(forked, 2), bits(forked, 0)), f"f={f} frame {s}: {name} of the copy differ from the source's"
            assert np.array_equal(bits(forked, 2), bits(control, 2)), f"f={f} frame {s}: {name} of the copy differ from the control's slot 2"
            assert np.array_equal(bits(forked, 0), bits(control, 0)), f"f={f} frame {s}: {name} of the source differ from the control's"
            assert np.array_equal(bits(forked, 1), bits(plain, 1)), f"f={f} frame {s}: {name} of session 1 changed"
    assert any(not np.array_equal(forked[s][1][2], plain[s][1][2]) for s in range(after)), "the fork changes nothing: nothing shown"


# ---- 9. the batcher -----------------------------------------------------------------------------------------------------------------------------
def check_batcher(device, lib, before=3, after=5):
    from moshi_amd.batcher import SessionBatcher
    from tests import batcher_cases as bc
    slots = 3
    mimi, lm, mcfg, lcfg = bc.tiny_pair(device, lib, slots)
    F = mcfg.frame_size
    rng = np.random.default_rng(SEED + 30)
    pcm = [(0.3 * rng.standard_normal(F)).astype(np.float32) for _ in range(before + after + 2)]

    def drain(b, ch):
        out = []
        while True:
            f = b.pop(ch)
            if f is None:
                return out
            out.append(f)
    with SessionBatcher(mimi, lm, slots, use_sampling=False) as b:
        parent = b.open()
        with pytest.raises(RuntimeError):              # MMI_ERR_STATE: opened since the last step, no state yet
            b.fork(parent)
        with pytest.raises(UnknownChannel):
            b.fork(parent + 1000)
        assert b.used_slots == 1
        for x in pcm[:before]:
            b.push(parent, x)
            assert b.step() == 1
        first = drain(b, parent)
        child = b.fork(parent)
        other = b.fork(parent, SessionSampling(temp=1.3, temp_text=1.2, top_k=60, top_k_text=25, seed=99))
        assert b.used_slots == 3 and len({parent, child, other}) == 3
        with pytest.raises(BufferError):               # MMI_ERR_BUSY
            b.fork(parent)
        assert b.used_slots == 3
        got = {parent: [], child: [], other: []}
        for x in pcm[before:before + after]:
            for ch in got:
                b.push(ch, x)
            assert b.step() == 3
            for ch in got:
                got[ch] += drain(b, ch)
        assert len(got[parent]) == len(got[child]) > 0 and len(first) <= before
        for i, ((pa, ta), (pb, tb)) in enumerate(zip(got[parent], got[child])):
            assert np.array_equal(ta, tb), f"frame {i}: the child's tokens differ from the parent's"
            assert np.array_equal(pa.view(np.uint8), pb.view(np.uint8)), f"frame {i}: the child's PCM differs from the parent's"
        assert any(not np.array_equal(ta, tb) for (_, ta), (_, tb) in zip(got[parent], got[other])), "a child with its own seed repeats the parent"
        b.close(parent)
        assert b.used_slots == 2
        for x in pcm[before + after:]:
            b.push(child, x)
            assert b.step() == 1
        assert len(drain(b, child)) == 2, "closing the parent stopped the child"
        again = b.open()                                # the parent's slot is free again
        assert b.used_slots == 3
        b.close(again)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------
def _fork_rc(call, handle, src, dst, n=None):
    arr = (C.c_int32 * max(len(dst), 1))(*dst)
    return int(call(handle, src, arr, len(dst) if n is None else n, None))


def check_refusals(device, lib):
    cfg, mcfg = tiny_lm_config(), tiny_mimi_config()
    B = 4
    lm = lm_of(device, lib, cfg, max_batch=B)
    mimi = MimiModel(random_mimi_state_dict(mcfg, seed=SEED), mcfg, device=device, max_batch=B, lib=lib)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    L = gen._lib
    bad = [(-1, [2]), (B, [2]), (1, [B]), (1, [-1]), (1, [1]), (1, [2, 1]), (1, [2, 3, 2]), (1, []), (0, list(range(1, 4)) * 6)]
    for call, handle, start, stop, snap in (
            (L.mmi_lm_fork_session, lm._handle, lambda: gen.streaming_forever(B), gen._stop_streaming, lambda: gen.get_streaming_state()["lm_gen"]),
            (L.mmi_mimi_fork_session, mimi._handle, lambda: mimi.streaming_forever(B), mimi._stop_streaming, lambda: mimi.get_streaming_state()["mimi"])):
        assert _fork_rc(call, handle, 0, [1]) == _capi.MMI_ERR_STATE, "not streaming"
        start()
        try:
            if handle is lm._handle:
                for c in codes_of(cfg, B, 3, SEED + 40):
                    take(gen, c, device)
            before = snap().cpu().numpy()
            for src, dst in bad:
                assert _fork_rc(call, handle, src, dst) == _capi.MMI_ERR_INVALID, (src, dst)
            assert _fork_rc(call, handle, 0, [1], n=17) == _capi.MMI_ERR_INVALID
            assert _fork_rc(call, handle, 0, [1], n=0) == _capi.MMI_ERR_INVALID
            assert np.array_equal(before, snap().cpu().numpy()), "a refused call changed the state"
            assert _fork_rc(call, handle, 0, [1, 3]) == _capi.MMI_OK
            assert not np.array_equal(before, snap().cpu().numpy()) or handle is not lm._handle
        finally:
            stop()
    with pytest.raises(ValueError):
        with gen.streaming(B):
            gen.fork_session(2, 2)
