"""Cases for the 4-bit KV ring (`kv_cache_dtype="fp4"`), shared by the simulator suite (tests/test_kv4_sim.py) and
the MI355X suite (tests/test_z_kv4_gpu.py).

The ring format, restated in numpy (`quantize` / `dequantize`): E2M1 codes (bit 3 sign, bits 2..0 the magnitude of
{0, .5, 1, 1.5, 2, 3, 4, 6}; two per byte, element 2i in the low nibble) under one E8M0 scale byte 2^(s - 127) per block of 16
consecutive head-dim elements.  s = E - 2 with E the biased exponent of the block's absmax (as bits: a NaN is the largest
magnitude), at most 253; E < 3: s = 0 and sixteen zero codes; round to nearest, ties to the even code; saturate at +-6; Inf and
NaN become +-6 under their sign.

The oracle (oracle/lm_oracle.py) rounds its ring inline; the 4-bit rounding sits here, in a subclass whose ring arrays quantise
on assignment (`Kv4Oracle`).  Two correct implementations of the network with this ring differ by rounding noise in the keys,
which flips a code now and then: measured 0.7 % of max|logit| in the worst case (mean 0.11 %) between the fp32 and the
accumulate64 oracle, against 0.35 % / 0.11 % with the bf16 ring - so the gates are the project's own, unchanged:
lm_cases.logits_close (5 % / 1.2 %) and lm_cases.near_tie."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import torch

from moshi_amd import LMGen, LMModel
from moshi_amd.config import tiny_lm_config
from oracle.lm_oracle import LMOracle
from tests import lm_cases
from tests.lm_cases import cached_lm_state_dict, logits_close, near_tie

MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def quantize(x: np.ndarray):
    """fp32 [..., 16 m] (bf16 values) -> (codes uint8 [..., 8 m], scale bytes uint8 [..., m])."""
    x = np.ascontiguousarray(x, np.float32)
    lead, n = x.shape[:-1], x.shape[-1]
    assert n % 16 == 0
    bits = x.view(np.uint32).reshape(lead + (n // 16, 16))
    mag = bits & np.uint32(0x7FFFFFFF)
    E = ((mag.max(-1) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    s = np.where(E < 3, 0, np.minimum(E - 2, 253))
    lim = np.where(s >= 253, 0x7F7FFFFF, ((s + 2) << 23) | 0x400000).astype(np.uint32)      # 6 * 2^(s - 127) where fp32 holds it
    clamped = np.minimum(mag, lim[..., None]).view(np.float32).astype(np.float64)
    q = np.ldexp(clamped, (127 - s)[..., None])                                               # |x| / 2^(s - 127), exact
    c = np.where(q < 2, np.rint(2 * q), np.where(q < 4, 2 + np.rint(q), 4 + np.rint(q / 2))).astype(np.uint8)
    c = np.where(mag >= np.uint32(0x7F800000), np.uint8(7), c)                                # Inf, NaN
    code = (((bits >> np.uint32(31)).astype(np.uint8) << 3) | c).astype(np.uint8)
    code = np.where((s == 0)[..., None], np.uint8(0), code)                                   # flushed block
    code = code.reshape(lead + (n // 2, 2))
    return (code[..., 0] | (code[..., 1] << 4)).astype(np.uint8), s.astype(np.uint8)


def dequantize(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """(codes [..., 8 m], scale bytes [..., m]) -> fp32 [..., 16 m]: code * 2^(s - 127), scale byte 0 = the factor 0."""
    lead, m = scales.shape[:-1], scales.shape[-1]
    nib = np.stack([codes & 15, codes >> 4], -1).reshape(lead + (m, 16))
    val = MAGNITUDES[nib & 7] * np.where(nib & 8, -1.0, 1.0)
    s = scales.astype(np.int64)[..., None]
    out = np.where(s == 0, 0.0, np.ldexp(val, s - 127))
    with np.errstate(over="ignore"):                 # s = 253 (a block that held an Inf or a NaN): codes 6 and 7 are 2^128 and up = Inf
        return out.reshape(lead + (16 * m,)).astype(np.float32)


def ring_round(x: np.ndarray) -> np.ndarray:
    return dequantize(*quantize(x))


class Kv4Ring(np.ndarray):
    """A ring array of the oracle that rounds what is written into it to the 4-bit format (blocks along the last axis)."""

    def __setitem__(self, key, value):
        super().__setitem__(key, ring_round(np.asarray(value, np.float32)))


class Kv4Oracle(LMOracle):
    def _streaming_model(self, B: int):
        super()._streaming_model(B)
        self.kv = [a.view(Kv4Ring) for a in self.kv]


def kv4_config(head_dim: int = 32, **kw):
    """tiny_lm_config with the 4-bit ring; head dim 64 / 128 through dim / num_heads."""
    shape = {32: dict(dim=128, num_heads=4), 64: dict(dim=128, num_heads=2), 128: dict(dim=256, num_heads=2)}[head_dim]
    return replace(tiny_lm_config(), kv_cache_dtype="fp4", **shape, **kw)


def bf16_bits_to_f32(u16: np.ndarray) -> np.ndarray:
    return (u16.astype(np.uint32) << np.uint32(16)).view(np.float32)


# ---- 1. the quantiser, exhaustively ------------------------------------------------------------------------------------------------------
ABSMAX = [1.0, 2.0 ** -20, 3.0, 0.0123, 448.0, 2.0 ** -124, 2.0 ** -125, float("inf"), 0.0]
# powers of two and others; 2^-124: E = 3, the smallest block that is kept (s = 1); 2^-125: E = 2 < 3, flushed wherever element 0
# is no larger; Inf; 0: the all-zero block is the row whose element 0 is +0


SWEPT = (0, 7, 10, 15)


def check_quantizer(lm: LMModel):
    """Every bf16 bit pattern as one element of a block (at each position of SWEPT) whose next element fixes the absmax: the device quantiser (the hardware's
    rounding and saturation on the GPU, the restatement on the simulator) equals the rule above bit for bit."""
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    am = torch.tensor(ABSMAX, dtype=torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    blocks = np.zeros((len(SWEPT), len(ABSMAX), 65536, 16), np.uint16)
    for i, pos in enumerate(SWEPT):                                 # the swept element at several places of the block: both
        blocks[i, :, :, pos] = pat                                  # words of codes, low and high nibbles
        blocks[i, :, :, (pos + 1) % 16] = am[:, None]
    rows = blocks.reshape(-1, 32)                                   # two blocks per row: m = 2
    codes, scales = lm.debug_kv4_quantize(torch.from_numpy(rows.view(np.int16)).view(torch.bfloat16))
    codes, scales = codes.cpu().numpy(), scales.cpu().numpy()
    want_c, want_s = quantize(bf16_bits_to_f32(rows))
    bad = np.nonzero(scales != want_s)
    assert not len(bad[0]), f"scale bytes differ at {bad[0][:5]}, {bad[1][:5]}: {scales[bad][:5]} against {want_s[bad][:5]}"
    bad = np.nonzero(codes != want_c)
    assert not len(bad[0]), (f"{len(bad[0])} code bytes differ, first at row {bad[0][0]} byte {bad[1][0]}: "
                             f"{codes[bad][:5]} against {want_c[bad][:5]}, input {rows[bad[0][0]]}")
    assert int(scales.max()) <= 253
    back = dequantize(codes, scales)
    assert not (back.view(np.uint32) & np.uint32(0xFFFF)).any(), "a dequantised value is no bf16 value"
    assert not np.isnan(back).any() and np.isfinite(back.reshape(-1, 16)[want_s.reshape(-1) <= 252]).all()   # Inf only where the input held one
    flushed = np.nonzero(want_s.reshape(-1) == 0)[0]
    assert len(flushed) and not want_c.reshape(-1, 8)[flushed].any()


# ---- 2. the ring's bytes -----------------------------------------------------------------------------------------------------------------
def split_planes(raw: np.ndarray, rows: int, cfg):
    H, Dh, cap = cfg.num_heads, cfg.dim // cfg.num_heads, cfg.context
    n = rows * H * cap
    assert raw.size == n * Dh // 2 + n * Dh // 16
    return raw[:n * Dh // 2].reshape(rows, H, cap, Dh // 2), raw[n * Dh // 2:].reshape(rows, H, cap, Dh // 16)


def check_ring_bytes(device, lib, cfg, B, steps=None, seed=31, quantize_weights=False, max_rows=None, stats=None, make=None):
    """A 4-bit handle and a bf16 twin on the same weights and forced tokens: layer 0's keys and values depend on the embeddings
    only, so the 4-bit planes of layer 0 must be the rule applied to the twin's bf16 ring, bit for bit, over every slot -
    with the ring wrapped.  make(sd, cfg, size) -> LMModel builds another kind of handle (fp8 linears, an adapter handle)."""
    steps = steps or cfg.context + 3
    sd = cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), seed)
    if quantize_weights == "mxfp4":
        from moshi_amd.weights import quantize_lm_state_dict_mxfp4
        sd = quantize_lm_state_dict_mxfp4(sd)
    elif quantize_weights:
        from moshi_amd.weights import quantize_lm_state_dict
        sd = quantize_lm_state_dict(sd)
    size = dict(max_rows=max_rows) if max_rows else dict(max_batch=B)
    make = make or (lambda sd_, cfg_, size_: LMModel(sd_, cfg_, device=device, lib=lib, **size_))
    gens = [LMGen(make(sd, replace(cfg, kv_cache_dtype=kv), size), use_sampling=False, support_out_of_sync=True) for kv in ("fp4", "bf16")]
    rng = np.random.default_rng(seed)
    H, Dh, cap = cfg.num_heads, cfg.dim // cfg.num_heads, cfg.context
    for g in gens:
        g.streaming_forever(B)
    try:
        for s in range(steps):
            codes = torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device)
            forced = np.concatenate([rng.integers(0, cfg.text_card, (B, 1)), rng.integers(0, cfg.card, (B, cfg.dep_q))], 1)
            for g in gens:
                g._step(codes, False, None, torch.from_numpy(forced).to(device))
            if s not in (cap // 2, steps - 1):
                continue
            for which in ("k", "v"):
                c4, s4 = split_planes(gens[0].kv_ring(0, which).cpu().numpy(), B, cfg)
                ref = gens[1].kv_ring(0, which).cpu().numpy().view(np.uint16).reshape(B, H, cap, Dh)
                want_c, want_s = quantize(bf16_bits_to_f32(ref))
                assert np.array_equal(s4, want_s), f"step {s} {which}: scale plane differs in {int((s4 != want_s).sum())} bytes"
                assert np.array_equal(c4, want_c), f"step {s} {which}: codes plane differs in {int((c4 != want_c).sum())} bytes"
                if s == steps - 1:
                    assert want_s.all(axis=-1).any() and want_c.any(), "the ring is empty: the case checks nothing"
        if stats is not None:
            stats["launch_list"] = list(gens[0].launch_list())
            stats["twin_launch_list"] = list(gens[1].launch_list())
    finally:
        for g in gens:
            g._stop_streaming()


# ---- 3. the network against the test-side oracle ------------------------------------------------------------------------------------------
def oracle_vs_engine(device, lib, cfg, seed, B, S, cfg_coef=1.0):
    """lm_cases.oracle_vs_engine's loop (masks, a partial reset at S // 2) with the 4-bit oracle; cfg_coef != 1: guided, two model
    rows per session (the text logits stay the conditioned row's: cfg_is_no_text, which needs no condition tensors), gates widened as for every guided comparison (lm_cases.GUIDED_WIDEN)."""
    sd = cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), seed)
    guided = cfg_coef != 1.0
    lm = LMModel(sd, cfg, device=device, max_batch=2 * B if guided else B, lib=lib)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=cfg_coef, cfg_is_no_text=guided)
    orc = Kv4Oracle(sd, cfg)
    orc.streaming(B, cfg_coef=cfg_coef, cfg_is_no_text=guided)
    widen = lm_cases.GUIDED_WIDEN if guided else 1.0
    rng = np.random.default_rng(seed)
    with gen.streaming(B):
        for s in range(S):
            mask = np.ones(B, bool)
            if B > 1:
                mask = rng.random(B) > 0.3
                mask[0] = True
                if s == S // 2:
                    r = np.zeros(B, bool); r[B - 1] = True
                    orc.reset_streaming(r); gen.reset_streaming(torch.from_numpy(r).to(device))
                    mask[B - 1] = True
            orc.set_exec_mask(mask); gen.set_exec_mask(torch.from_numpy(mask).to(device))
            codes = rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))
            oo, (otl, oal, ott, oat) = orc.step(codes, use_sampling=False, support_out_of_sync=True)
            forced = np.concatenate([ott[:, None], oat], 1)
            out, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device), forced_tokens=torch.from_numpy(forced).to(device))
            out, tl, al = out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy()
            for b in range(B):
                if not mask[b]:
                    continue
                assert np.array_equal(out[b], oo[b]), f"step {s} row {b}: ring output differs"
                assert logits_close(tl[b], otl[b], widen), f"step {s} row {b}: text logits {np.abs(tl[b] - otl[b]).max()}"
                for k in range(cfg.dep_q):
                    assert logits_close(al[b, k], oal[b, k], widen), f"step {s} row {b} cb {k}: {np.abs(al[b, k] - oal[b, k]).max()}"
                    a_e, a_o = int(al[b, k].argmax()), int(oat[b, k])
                    assert a_e == a_o or near_tie(oal[b, k], a_e, a_o, widen)


# ---- 4. a long ring ------------------------------------------------------------------------------------------------------------------------
_LONG = {}


def long_ring_reference(cfg, sd, steps, seed):
    """The oracle's run of the long-ring case, computed once and shared by the paths that replay it (left unchanged)."""
    key = (repr(cfg), steps, seed)
    if key not in _LONG:
        orc = Kv4Oracle(sd, cfg)
        orc.streaming(1)
        rng = np.random.default_rng(seed)
        trace = []
        for s in range(steps):
            codes = rng.integers(0, cfg.card, (1, cfg.n_q - cfg.dep_q, 1))
            oo, (otl, oal, ott, oat) = orc.step(codes, use_sampling=False, support_out_of_sync=True)
            trace.append((codes, oo.copy(), otl.copy(), oal.copy(), np.concatenate([ott[:, None], oat], 1)))
        _LONG.clear()
        _LONG[key] = trace
    return _LONG[key]


def check_long_ring(device, lib, context=600, steps=300, every=20, last=10, seed=44):
    """test_long_ring_split_over_workgroups_matches_oracle for the 4-bit ring: one session, `steps` positions deep, read back
    every `every`-th step and the last `last`."""
    cfg = replace(tiny_lm_config(), context=context, kv_cache_dtype="fp4")
    sd = cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), seed)
    gen = LMGen(LMModel(sd, cfg, device=device, max_batch=1, lib=lib), use_sampling=False, support_out_of_sync=True)
    with gen.streaming(1):
        for s, (codes, oo, otl, oal, forced) in enumerate(long_ring_reference(cfg, sd, steps, seed)):
            forced = torch.from_numpy(forced).to(device)
            if s % every and s < steps - last:
                gen._step(torch.from_numpy(codes).to(device), False, None, forced)
                continue
            out, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device), forced_tokens=forced)
            assert np.array_equal(out.cpu().numpy(), oo), f"step {s}"
            assert logits_close(tl[0].cpu().numpy(), otl[0]), f"step {s}: text logits"
            for k in range(cfg.dep_q):
                assert logits_close(al[0, k].cpu().numpy(), oal[0, k]), f"step {s} cb {k}"


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------------
def check_repeat_streams(device, lib, B, steps=14, seed=77):
    """The same stream twice on one handle: tokens, logits and hidden taps bit-identical (the ring wraps: steps > context)."""
    cfg = kv4_config()
    sd = cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), seed + B)
    gen = LMGen(LMModel(sd, cfg, device=device, max_batch=B, lib=lib), use_sampling=False, support_out_of_sync=True)
    gen.lm_model.enable_hidden_taps()
    rng = np.random.default_rng(seed)
    plan = []
    for s in range(steps):
        mask = rng.random(B) > 0.3
        mask[0] = True
        reset = None
        if s == 1 and B > 1:
            reset = np.zeros(B, bool); reset[B - 1] = True
        plan.append((mask, reset, rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))))

    def run():
        out = []
        with gen.streaming(B):
            for mask, reset, codes in plan:
                if reset is not None:
                    gen.reset_streaming(torch.from_numpy(reset).to(device))
                gen.set_exec_mask(torch.from_numpy(mask).to(device))
                o, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device))
                out.append((o.cpu(), tl.cpu(), al.cpu(), gen.hidden_taps().cpu()))
        return out
    first, again = run(), run()
    for s, (a, b) in enumerate(zip(first, again)):
        m = torch.from_numpy(plan[s][0])
        for name, x, y in zip(("tokens", "text logits", "audio logits"), a[:3], b[:3]):
            assert torch.equal(x[m], y[m]), f"step {s}: {name} differ between two streams fed the same frames"
        for w in (0, 1):
            assert torch.equal(a[3][w][m], b[3][w][m]), f"step {s}: the residual stream (tap {w}) differs"


# ---- 6. snapshots and sizes ----------------------------------------------------------------------------------------------------------------
def check_sizes_and_snapshot(device, lib, B=8):
    cfg = kv4_config()
    sd = cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), 21)
    elems = 2 * cfg.num_layers * B * cfg.dim * cfg.context                 # keys + values, every layer
    per_layer = elems // (2 * cfg.num_layers)                             # a 4-bit layer: codes + scale bytes, padded to 256 bytes
    ring = {"bf16": 2 * elems, "fp8": elems, "fp4": 2 * cfg.num_layers * ((per_layer // 2 + per_layer // 16 + 255) // 256 * 256)}
    assert ring["fp4"] == elems // 2 + elems // 16                        # (no padding at this shape: 0.5625 bytes per element)
    size = {}
    for kv in ("bf16", "fp8", "fp4"):
        gen = LMGen(LMModel(sd, replace(cfg, kv_cache_dtype=kv), device=device, max_batch=B, lib=lib), use_sampling=False, support_out_of_sync=True)
        with gen.streaming(B):
            size[kv] = int(gen._lib.mmi_lm_state_bytes(gen.lm_model._handle))
            if kv != "fp4":
                assert gen.kv_ring(0, "k").numel() == ring[kv] // (2 * cfg.num_layers)      # the copy works for every ring
                continue
            for l in range(cfg.num_layers):                       # both planes zeroed by streaming_start
                for which in ("k", "v"):
                    raw = gen.kv_ring(l, which)
                    assert raw.numel() == ring["fp4"] // (2 * cfg.num_layers) and not raw.any()
            rng = np.random.default_rng(5)
            frames = [torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device) for _ in range(cfg.context + 4)]

            def run(fs):
                return [tuple(t.clone() for t in gen.step_with_taps(x)) for x in fs]
            run(frames[:-3])                                       # the ring has wrapped
            snap = gen.get_streaming_state()
            assert snap["lm_gen"].numel() == size["fp4"]
            first = run(frames[-3:])
            gen.set_streaming_state(snap)
            again = run(frames[-3:])
            for a, b in zip(first, again):
                for x, y in zip(a, b):
                    assert torch.equal(x, y), "the continuation after a restored snapshot differs"
            assert gen.kv_ring(0, "k").any() and gen.kv_ring(1, "v").any()
    assert size["bf16"] - size["fp4"] == ring["bf16"] - ring["fp4"], (size, ring)
    assert size["fp8"] - size["fp4"] == ring["fp8"] - ring["fp4"], (size, ring)


# ---- 7. API and refusals -------------------------------------------------------------------------------------------------------------------
def check_api_and_refusals(device, lib):
    import pytest
    from moshi_amd.config import LMConfig
    cfg = tiny_lm_config()
    sd = cached_lm_state_dict(cfg, 21)
    assert LMModel(sd, cfg, device=device, max_batch=2, lib=lib, kv_cache="fp4").config.kv_cache_dtype == "fp4"
    assert LMModel(sd, replace(cfg, kv_cache_dtype="fp4"), device=device, max_batch=2, lib=lib).config.kv_cache_dtype == "fp4"
    assert LMConfig(kv_cache_dtype="fp4").kv_cache_dtype == "fp4"
    odd = replace(cfg, dim=96, num_heads=2)                      # head dim 48
    with pytest.raises(ValueError, match="multiple of 32"):
        LMModel(cached_lm_state_dict(odd, 22), odd, device=device, max_batch=2, lib=lib, kv_cache="fp4")
    for bad in ("fp16", "e2m1", "int4", ""):
        with pytest.raises(ValueError, match="kv_cache_dtype must be"):
            LMModel(sd, cfg, device=device, max_batch=2, lib=lib, kv_cache=bad)


def check_abi_refuses_odd_head_dim(device, lib):
    """The C ABI's own refusal (mmi_lm_cfg.kv_cache_dtype = MMI_F4E2M1X2 at a head dim of 48): MMI_ERR_UNSUPPORTED with the reason."""
    import pytest
    from moshi_amd import _capi, lm as lm_mod
    odd = replace(tiny_lm_config(), dim=96, num_heads=2)
    sd = cached_lm_state_dict(odd, 22)
    real = lm_mod._lm_cfg_struct

    def forged(cfg):
        s = real(cfg)
        s.kv_cache_dtype = _capi.MMI_F4E2M1X2
        return s
    lm_mod._lm_cfg_struct = forged
    try:
        with pytest.raises(NotImplementedError, match="head dim multiple of 32"):
            LMModel(sd, odd, device=device, max_batch=2, lib=lib)
    finally:
        lm_mod._lm_cfg_struct = real


def check_batcher(device, lib):
    """SessionBatcher on a 4-bit-ring LM: batcher_cases' by-hand schedule check at 3 slots."""
    from moshi_amd import MimiModel, SessionBatcher
    from moshi_amd.config import tiny_mimi_config
    from moshi_amd.weights import random_lm_state_dict, random_mimi_state_dict
    from tests import batcher_cases as bc
    slots = 3
    lcfg = kv4_config()
    mcfg = replace(tiny_mimi_config(), q_bins=lcfg.card, q_n_q=lcfg.dep_q)

    def pair():
        mimi = MimiModel(random_mimi_state_dict(mcfg, seed=5), mcfg, device=device, max_batch=slots, num_codebooks=lcfg.dep_q, lib=lib)
        return mimi, LMModel(random_lm_state_dict(lcfg, seed=6), lcfg, device=device, max_batch=slots, lib=lib)
    mimi_a, lm_a = pair()
    manual = bc.ManualLoop(*pair(), slots)
    with SessionBatcher(mimi_a, lm_a, slots, use_sampling=False) as batcher:
        res, ref = bc.scripted_run(batcher, manual, mcfg.frame_size)
        st = batcher.stats()
    manual.stop()
    assert st["steps"] == bc.N_STEPS and st["dropped_frames"] == 0
    played = 0
    for s in res:
        assert len(res[s]) == len(ref[s]), f"session {s}: {len(res[s])} frames from the batcher, {len(ref[s])} by hand"
        for i, ((pa, ta), (pb, tb)) in enumerate(zip(res[s], ref[s])):
            assert np.array_equal(ta, tb), f"session {s} frame {i}: tokens differ"
            assert np.array_equal(pa, pb), f"session {s} frame {i}: PCM differs"
        played += len(res[s])
    assert played > 8
