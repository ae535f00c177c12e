"""The layout of the LM engine's streaming state, pinned (tests/golden/lm_state_layout.json), shared by the simulator test
(tests/test_state_layout_sim.py) and the GPU test (tests/test_b_state_layout_gpu.py).

A snapshot (`mmi_lm_state_save`) is the streaming-state arena in allocation order, so that order and every buffer's size are a
wire format.  Per configuration the golden file holds, taken on the commit BEFORE the state table existed (its simulator
library, MMI_DEBUG_POISON=1: every allocation starts as 0xFF bytes, so a buffer that `streaming_start` does not initialise
stays 0xFF and the hash tells which buffers are initialised and with what):

    state_bytes      mmi_lm_state_bytes
    regions          the text of mmi_lm_debug_state_regions (its `scratch<i>` lines carry the arena index and size of every buffer)
    start_sha256     sha256 of the snapshot right after streaming_start
    step_sha256      sha256 of the snapshot after STEPS steps on seeded inputs (simulator only)
    launch_sha256    sha256 of the text of mmi_lm_launch_list after those steps (but for one field of its first line: measure())

The configurations are the tiny models of the other case files at the smallest row counts that reach every branch of the
table's builder (guidance, masked_until, a summed condition, cross-attention under a capacity, hidden taps, int8 activations, the
nucleus tail, the TTS rows, the adapter slots) and every ring form."""
from __future__ import annotations

import hashlib
import json
import os
from dataclasses import replace
from pathlib import Path

import numpy as np
import torch

from moshi_amd import _capi
from moshi_amd.config import tiny_lm_config
from moshi_amd.lm import ConditionFuser, LMGen, LMModel
from tests import mxfp4_cases as mx
from tests import row_condition_cases as rc
from tests import tts_machine_cases as tm
from tests.lm_cases import cached_lm_state_dict
from tests.many_rows_cases import env

GOLDEN = Path(__file__).resolve().parent / "golden" / "lm_state_layout.json"
SEED = 57
STEPS = 3


def _tiny(device, lib, B, max_batch, gen_kw=None, cfg=None, **model_kw):
    cfg = cfg or tiny_lm_config()
    lm = LMModel(cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), SEED), cfg, device=device, max_batch=max_batch, lib=lib, **model_kw)
    return LMGen(lm, use_sampling=False, support_out_of_sync=True, **(gen_kw or {})), B


def _guided(device, lib):
    cfg = tiny_lm_config()
    g = torch.Generator().manual_seed(SEED)
    cs = (0.5 * torch.randn(4, 1, cfg.dim, generator=g)).to(torch.bfloat16)
    kw = dict(cfg_coef=2.0, cfg_is_masked_until=[1, 2], condition_tensors={"c": (cs, torch.ones(4, 1, dtype=torch.bool))})
    return _tiny(device, lib, 2, 4, gen_kw=kw, fuser=ConditionFuser({"sum": ["c"]}))


def _cross(device, lib):
    cfg = rc.tiny_cross_config()
    conds = rc.tensors([rc.session_cond(cfg, b, 3, 1) for b in range(2)])
    return _tiny(device, lib, 2, 2, gen_kw=dict(condition_tensors=conds), cfg=cfg, cross_capacity=5, fuser=ConditionFuser({"sum": ["s"], "cross": ["x"]}))


def _taps(device, lib):
    gen, B = _tiny(device, lib, 2, 2)
    gen.lm_model.enable_hidden_taps()
    return gen, B


def _tts(device, lib):
    return tm.tts_gen(device, lib, tm.machine_of(tm.golden("tts_machine.npz")["params"], 2)), 3


def _nucleus(device, lib):
    gen, B = _tiny(device, lib, 2, 2, gen_kw=dict(top_p=0.9, top_p_text=0.8, seed=SEED))
    gen.use_sampling = True
    return gen, B


# name -> (environment at handle creation, (device, lib) -> (LMGen not yet streaming, sessions))
CONFIGS = {
    "bf16_b2": ({}, lambda d, l: _tiny(d, l, 2, 2)),                                   # 16-row tile
    "bf16_b17": ({}, lambda d, l: _tiny(d, l, 17, 32)),                                # 32-row tile
    "bf16_b17_dep_tile16": ({"MMI_DEP_TILE": "16"}, lambda d, l: _tiny(d, l, 17, 32)),
    "guided_masked_until_sum": ({}, _guided),
    "cross_len3_cap5": ({}, _cross),
    "int8_act8": ({}, lambda d, l: _tiny(d, l, 2, 2, quantize=True)),
    "kv_fp8": ({}, lambda d, l: _tiny(d, l, 2, 2, kv_cache="fp8")),
    "kv_fp4": ({}, lambda d, l: _tiny(d, l, 2, 2, kv_cache="fp4")),
    "nucleus": ({}, _nucleus),
    "tts_machine": ({}, _tts),
    "adapters": ({}, lambda d, l: _tiny(d, l, 2, 2, adapters=(2, 32))),
    "hidden_taps": ({}, _taps),
    "prefill32_score": ({}, lambda d, l: _tiny(d, l, 2, 2, prefill_rows=32, score=True)),
    # the launch forms the configurations above never reach: a split-K partial GEMM and its fold in the next norm launch, fp8 and
    # MXFP4 weights, the int8 x int8 path with the norm and quantisation launches of their own (and its int32 partials), k_gemm_rows
    # (recorded on the parent of the commit that added them, like the others: profiles/gemm_args/README.md)
    "bf16_b2_ksplit2": ({"MMI_GEMM_KSPLIT": "2"}, lambda d, l: _tiny(d, l, 2, 2)),
    "fp8": ({}, lambda d, l: _tiny(d, l, 2, 2, quantize="fp8")),
    "mxfp4": ({}, lambda d, l: _tiny(d, l, 2, 2, cfg=mx.mx_config(), quantize="mxfp4")),
    "int8_unfused": ({"MMI_NO_NORM_FUSION": "1"}, lambda d, l: _tiny(d, l, 2, 2, quantize=True)),
    "int8_unfused_ksplit2": ({"MMI_NO_NORM_FUSION": "1", "MMI_GEMM_KSPLIT": "2"}, lambda d, l: _tiny(d, l, 2, 2, quantize=True)),
    "bf16_rows65": ({}, lambda d, l: _tiny(d, l, 65, 32, max_rows=65)),                # three batch tiles
}
# `xkv` comes out of a GEMM: its bytes are the device's arithmetic, not a fill or a host copy
GEMM_AT_START = ("cross_len3_cap5", "tts_machine")


def _sha(gen) -> str:
    return hashlib.sha256(gen.get_streaming_state()["lm_gen"].cpu().numpy().tobytes()).hexdigest()


def measure(name, device, lib, steps=True) -> dict:
    """The recorded values of configuration `name` on (device, lib); steps=False: without step_sha256."""
    env_kw, make = CONFIGS[name]
    tm._MODELS.clear()                  # (tts_machine_cases caches its model per library: the poison knob is read at create)
    with env(MMI_DEBUG_POISON="1", **env_kw):
        gen, B = make(device, lib)
    handle, cdll = gen.lm_model._handle, gen._lib
    out = {}
    gen.streaming_forever(B)
    try:
        out["state_bytes"] = int(cdll.mmi_lm_state_bytes(handle))
        out["regions"] = _capi.read_text(lambda buf, cap: cdll.mmi_lm_debug_state_regions(handle, buf, cap))
        out["start_sha256"] = _sha(gen)
        cfg = gen.lm_model.config
        rng = np.random.default_rng(SEED)
        for _ in range(STEPS):
            gen.step(torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device))
        if steps:
            out["step_sha256"] = _sha(gen)
        text = _capi.read_text(lambda buf, cap: cdll.mmi_lm_launch_list(handle, buf, cap))
        assert text, "no launch list after a step"
        # The whole text, per-launch weight bytes included, but for the bytes field of the FIRST line: the recorder
        # (api_common.hip) keeps the bytes a GEMM announced outside a recording - a later step, a prefill pass, a debug tap - and
        # charges them to the first launch of the next list recorded on that thread.  That launch is k_lm_prepare, which streams no
        # weights, so the field is what the thread ran before and never a property of this stream.
        first, _, rest = text.partition("\n")
        assert first.split("\t")[:2] == ["prepare", "k_lm_prepare"], first
        text = "\t".join(first.split("\t")[:2]) + "\n" + rest
        out["launch_sha256"] = hashlib.sha256(text.encode()).hexdigest()
        out["launch_text"] = text
    finally:
        gen._stop_streaming()
        tm._MODELS.clear()
    return out


def load_golden() -> dict:
    return json.loads(GOLDEN.read_text())


def check(name, device, lib, on_device=False):
    """Every recorded value of `name`.  on_device: a real GPU - no step hash (the device's arithmetic is not the simulator's), the
    start hash where no GEMM runs at the start, and the device's own launch list where the golden file records one."""
    want = load_golden()[name]
    got = measure(name, device, lib, steps=not on_device)
    knobs = {k: v for k, v in os.environ.items() if k.startswith(("MMI_", "HIPSIM_"))}
    for k, v in got.items():      # (shown when an assertion below fails: the texts themselves, and the knobs the handle was created under)
        print(f"{name}: {k} = {v}")
    print(f"{name}: environment {knobs}")
    assert got["state_bytes"] == want["state_bytes"], f"{name}: mmi_lm_state_bytes {got['state_bytes']}, recorded {want['state_bytes']}"
    assert got["regions"] == want["regions"], f"{name}: the regions text differs from the recorded one"
    if not on_device or name not in GEMM_AT_START:
        assert got["start_sha256"] == want["start_sha256"], f"{name}: the snapshot right after streaming_start differs"
    if not on_device:
        assert got["step_sha256"] == want["step_sha256"], f"{name}: the snapshot after {STEPS} steps differs"
    launch = want.get("device_launch_sha256", want["launch_sha256"]) if on_device else want["launch_sha256"]
    assert got["launch_sha256"] == launch, f"{name}: the launch list differs from the recorded one"
