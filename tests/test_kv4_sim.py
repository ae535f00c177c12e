"""The 4-bit KV ring (`kv_cache_dtype="fp4"`) on the CPU kernel simulator: tests/kv4_cases.py against the engine's
host restatement of the conversions and the same kernel code the GPU runs."""
import os
import subprocess
import sys
from dataclasses import replace
from pathlib import Path

import pytest

from moshi_amd import LMModel
from tests import kv4_cases as kc
from tests.lm_cases import cached_lm_state_dict

ROOT = Path(__file__).resolve().parent.parent


def in_proj_kernels(launch_list):
    return {k for site, k in launch_list if site == "L.in_proj" and "k_gemm" in k}


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------------
def test_quantiser_equals_the_rule_on_every_bf16_pattern(sim_lib):
    cfg = kc.kv4_config()
    kc.check_quantizer(LMModel(cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), 21), cfg, device="cpu", max_batch=2, lib=sim_lib))


def test_numpy_rule_rounds_ties_to_the_even_code_and_saturates():
    import numpy as np
    x = np.zeros((1, 16), np.float32)
    x[0, :10] = [4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, -5.1]        # absmax 6: E = 129, s = 127, scale 1
    codes, scales = kc.quantize(x)
    assert scales[0, 0] == 127
    nib = np.stack([codes[0] & 15, codes[0] >> 4], -1).reshape(-1)
    assert list(nib[:10]) == [6, 0, 2, 2, 4, 4, 6, 6, 7, 8 | 7]                 # ties: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    assert np.array_equal(kc.dequantize(codes, scales)[0, :3], [4.0, 0.0, 1.0])


# ---- 2. the ring's bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,head_dim,max_rows", [(1, 32, None), (17, 64, None), (33, 128, None), (65, 32, 65)])
def test_ring_planes_equal_the_rule_applied_to_the_bf16_twin(sim_lib, B, head_dim, max_rows):
    """16-row tile, 32-row tile, two batch tiles, k_gemm_rows; head dims 32 / 64 / 128; the ring wraps (steps > context)."""
    st = {}
    kc.check_ring_bytes("cpu", sim_lib, kc.kv4_config(head_dim, context=5), B, max_rows=max_rows, stats=st)
    if max_rows:
        assert any("k_gemm_rows" in k for k in in_proj_kernels(st["launch_list"]))


def test_ring_planes_under_the_row_group_control(sim_lib, monkeypatch):
    """MMI_ROWS_GROUPS=1: a 65-row handle launched as one <= 64-row GEMM per row group - the second group's view of the ring moves
    the codes plane and the scale plane by different strides (rows_group_view)."""
    monkeypatch.setenv("MMI_ROWS_GROUPS", "1")
    st = {}
    kc.check_ring_bytes("cpu", sim_lib, kc.kv4_config(context=5), 65, steps=6, max_rows=65, stats=st)
    assert not any("k_gemm_rows" in k for k in in_proj_kernels(st["launch_list"]))


@pytest.mark.parametrize("form", ["xlds-8", "xlds-5", "once", "osplit-4a", "osplit-4a-16", "int8", "fp8w", "mxfp4", "lora"])
def test_ring_planes_through_every_in_proj_form(sim_lib, monkeypatch, form):
    """The kernels that share the epilogue and can run in_proj.  xlds-8: 12 in_proj tiles over 8 workgroups = 6 octets each, every
    share starts on an even octet (the production split); xlds-5: uneven shares that would cut a 16-element block - the 4-bit
    in_proj stays on k_gemm_xp; osplit-4a: four parts asked for - a 4-bit in_proj takes two (whole octet pairs) at the 32-row
    tile and none at the 16-row tile; the weight forms; the LoRA tail."""
    B, qw, cfg = 18, False, kc.kv4_config(context=5)
    if form.startswith("xlds"):
        monkeypatch.setenv("MMI_GEMM_LDS", "2")
        monkeypatch.setenv("MMI_GEMM_LDS_GRID", form.split("-")[1])
    elif form == "once":
        monkeypatch.setenv("MMI_GEMM_ONCE", "a")
        monkeypatch.setenv("MMI_GEMM_LDS", "0")
    elif form.startswith("osplit"):
        monkeypatch.setenv("MMI_GEMM_OSPLIT", "4a")
        B = 3 if form.endswith("16") else 18
    elif form == "int8":
        qw = True
    elif form == "mxfp4":
        qw, cfg = "mxfp4", replace(cfg, card=72, depformer_dim_feedforward=240)      # every in_features a multiple of 32 (mxfp4_cases.mx_config)
    st = {}
    if form == "fp8w":
        check_fp8_weights(sim_lib, cfg, B)
        return
    if form == "lora":
        check_lora_handle(sim_lib, cfg, B)
        return
    kc.check_ring_bytes("cpu", sim_lib, cfg, B, quantize_weights=qw, stats=st)
    ks = in_proj_kernels(st["launch_list"])
    if form == "xlds-8":
        assert any("k_gemm_xlds" in k for k in ks), ks
    if form == "xlds-5":
        assert not any("k_gemm_xlds" in k for k in ks) and any("k_gemm_xlds" in k for k in in_proj_kernels(st["twin_launch_list"])), ks
    if form == "once":
        assert any("k_gemm_xp_once" in k for k in ks), ks


def check_fp8_weights(lib, cfg, B):
    """e4m3 linears: the ring bytes against the twin with the same fp8 tensors."""
    from moshi_amd.weights import quantize_lm_state_dict_fp8
    kc.check_ring_bytes("cpu", lib, cfg, B, make=lambda sd, c, size: LMModel(quantize_lm_state_dict_fp8(sd), c, device="cpu", lib=lib, **size))


def check_lora_handle(lib, cfg, B):
    """An adapter handle (every linear on the LORA form of k_gemm_xp, shrink launch in front): no adapter loaded, the tail adds +0."""
    kc.check_ring_bytes("cpu", lib, cfg, B, make=lambda sd, c, size: LMModel(sd, c, device="cpu", lib=lib, adapters=(2, 32), **size))


# ---- 3. the network against the test-side oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,head_dim,context", [(1, 15, 32, 12), (5, 16, 128, 12), (17, 5, 32, 3), (33, 5, 128, 3)])
def test_network_matches_the_4_bit_oracle(sim_lib, B, S, head_dim, context):
    """S > context everywhere: the ring wraps (a ring of 3 slots at the larger batches keeps the cases short)."""
    kc.oracle_vs_engine("cpu", sim_lib, kc.kv4_config(head_dim, context=context), seed=50 + B, B=B, S=S)


def test_guided_network_matches_the_4_bit_oracle(sim_lib):
    kc.oracle_vs_engine("cpu", sim_lib, kc.kv4_config(), seed=58, B=3, S=14, cfg_coef=2.0)


# ---- 4. the ring shared out over workgroups -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["wave", "wave-solo", "wave-switch", "wave-kernel", "split"])
def test_attention_ring_split_over_several_workgroups(sim_lib, monkeypatch, kernel):
    """test_lm_sim.py's split-ring paths (both attention kernels; solo program, graph switch, merge launch, merge in the kernel)
    at its depth, with the ring wrapping."""
    monkeypatch.setenv("MMI_ATTN_NS", "3")
    monkeypatch.setenv("MMI_ATTN", kernel.split("-")[0])
    monkeypatch.setenv("MMI_ATTN_SOLO", {"wave-solo": "768", "wave-switch": "4"}.get(kernel, "0"))
    if kernel == "wave-kernel":
        monkeypatch.setenv("MMI_ATTN_MERGE", "kernel")
    kc.oracle_vs_engine("cpu", sim_lib, kc.kv4_config(), seed=61, B=2, S=15)


def test_ring_longer_than_one_chunk_of_the_chunked_kernel(sim_lib, monkeypatch):
    """300 slots: more than one 256-slot chunk of k_lm_attn_split and five row groups per wave of k_lm_attn_wave at head dim 32."""
    kc.check_long_ring("cpu", sim_lib, context=300, steps=40, every=13, last=2)
    monkeypatch.setenv("MMI_ATTN", "split")
    kc.check_long_ring("cpu", sim_lib, context=300, steps=30, every=29, last=1)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 18])
def test_repeat_streams_are_bit_identical(sim_lib, B):
    kc.check_repeat_streams("cpu", sim_lib, B)


_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import build_sim
from moshi_amd import _capi
from tests import kv4_cases as kc
kc.check_repeat_streams("cpu", _capi.load(build_sim.build()), int(sys.argv[2]))
print("ok")
"""


@pytest.mark.parametrize("sched", ["reverse", "random:7"])
def test_repeat_streams_under_other_workgroup_schedules(sim_lib, tmp_path, sched):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    p = subprocess.run([sys.executable, str(script), str(ROOT), "18"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, HIPSIM_SCHED=sched))
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]


# ---- 6. snapshots and sizes; 7. API ---------------------------------------------------------------------------------------------------------
def test_state_bytes_snapshot_and_zeroed_planes(sim_lib):
    kc.check_sizes_and_snapshot("cpu", sim_lib)


def test_api_and_refusals(sim_lib):
    kc.check_api_and_refusals("cpu", sim_lib)
    kc.check_abi_refuses_odd_head_dim("cpu", sim_lib)


def test_batcher_on_a_4_bit_ring_equals_the_hand_driven_schedule(sim_lib):
    kc.check_batcher("cpu", sim_lib)


def test_header_prototypes_equal_the_ctypes_signatures():
    import ctypes as C
    import re
    from moshi_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "moshi_mi.h").read_text(), flags=re.S)
    assert re.search(r"int mmi_lm_debug_kv4_quantize\(mmi_lm\* lm, const void\* x_bf16, int32_t n, int32_t m, void\* codes_u8, void\* scales_u8, "
                     r"mmi_stream stream\);", text)
    assert re.search(r"int64_t mmi_lm_debug_kv_ring\(mmi_lm\* lm, int32_t layer, int32_t which, void\* dst, int64_t nbytes, mmi_stream stream\);", text)
    P = C.c_void_p
    assert _capi.SIGNATURES["mmi_lm_debug_kv4_quantize"] == (C.c_int, [P, P, C.c_int32, C.c_int32, P, P, P])
    assert _capi.SIGNATURES["mmi_lm_debug_kv_ring"] == (C.c_int64, [P, C.c_int32, C.c_int32, P, C.c_int64, P])
    assert _capi.MMI_F4E2M1X2 == 6
