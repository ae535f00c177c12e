"""The 4-bit KV ring (`kv_cache_dtype="fp4"`) on a real MI355X: tests/kv4_cases.py against the hardware's own
conversions (v_cvt_scalef32_pk_fp4_f32 / v_cvt_scalef32_pk_f32_fp4).  Collected after the core-path files."""
from dataclasses import replace

import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import kv4_cases as kc
from tests.lm_cases import cached_lm_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"


def in_proj_kernels(launch_list):
    return {k for site, k in launch_list if site == "L.in_proj" and "k_gemm" in k}


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------------
def test_hardware_quantiser_equals_the_rule_on_every_bf16_pattern(gpu_lib):
    cfg = kc.kv4_config()
    kc.check_quantizer(LMModel(cached_lm_state_dict(replace(cfg, kv_cache_dtype="bf16"), 21), cfg, device=DEV, max_batch=2))


# ---- 2. the ring's bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,head_dim,max_rows", [(1, 32, None), (17, 32, None), (33, 32, None), (65, 32, 65), (17, 64, None), (33, 128, None),
                                                 (1, 128, None)])
def test_ring_planes_equal_the_rule_applied_to_the_bf16_twin(gpu_lib, B, head_dim, max_rows):
    """16-row tile, 32-row tile, two batch tiles, k_gemm_rows (max_rows=65); head dims 32 / 64 / 128; the ring wraps."""
    st = {}
    kc.check_ring_bytes(DEV, None, kc.kv4_config(head_dim), B, max_rows=max_rows, stats=st)
    if max_rows:
        assert any("k_gemm_rows" in k for k in in_proj_kernels(st["launch_list"]))


def production_config():
    """One temporal layer at the 7B in_proj shape (dim 4096, 32 heads of 128), context 8; the rest stays tiny."""
    return replace(tiny_lm_config(), dim=4096, num_heads=32, num_layers=1, context=8, hidden_scale=4.0, kv_cache_dtype="fp4")


@pytest.mark.parametrize("B,weights", [(32, "bf16"), (64, "bf16"), (32, "mxfp4"), (64, "int8")])
def test_ring_planes_under_the_production_in_proj_plans(gpu_lib, B, weights):
    """384 in_proj tiles: bf16 weights take k_gemm_xlds (6 row octets per workgroup: every share starts on an even octet, so no
    16-element block is cut), one and two batch tiles; MXFP4 and int8 x int8 linears stay on k_gemm_xp."""
    cfg = production_config()
    if weights == "mxfp4":
        cfg = replace(cfg, card=72, depformer_dim_feedforward=240)       # every in_features a multiple of 32
    st = {}
    kc.check_ring_bytes(DEV, None, cfg, B, quantize_weights={"bf16": False, "mxfp4": "mxfp4", "int8": True}[weights], stats=st)
    ks = in_proj_kernels(st["launch_list"])
    assert ks, st["launch_list"]
    if weights == "bf16":
        assert all("k_gemm_xlds" in k for k in ks), ks
    else:
        assert ks == {"k_gemm_xp"}, ks
    assert ks == in_proj_kernels(st["twin_launch_list"]), "the 4-bit handle planned in_proj differently from its bf16 twin"


# ---- 3. the network against the test-side oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,head_dim,context", [(1, 16, 32, 12), (5, 16, 128, 12), (17, 5, 32, 3), (33, 5, 128, 3), (5, 16, 32, 12),
                                                  (17, 5, 128, 3)])
def test_network_matches_the_4_bit_oracle(gpu_lib, B, S, head_dim, context):
    """Masks, a partial reset at S // 2; S > context everywhere: the ring wraps (3 slots at the larger batches keep the oracle short)."""
    kc.oracle_vs_engine(DEV, None, kc.kv4_config(head_dim, context=context), seed=50 + B, B=B, S=S)


def test_guided_network_matches_the_4_bit_oracle(gpu_lib):
    kc.oracle_vs_engine(DEV, None, kc.kv4_config(), seed=58, B=3, S=14, cfg_coef=2.0)


# ---- 4. a long ring ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["switch", "launch"])
def test_long_ring_split_over_workgroups_matches_oracle(gpu_lib, monkeypatch, path):
    """test_b_lm_gpu.py's long-ring case for the 4-bit ring, 300 positions deep: "switch" runs the solo program (graph), then goes
    over to the split over workgroups with the combine launch after 100 steps; "launch" takes that program from the first row."""
    monkeypatch.setenv("MMI_ATTN_SOLO", "100" if path == "switch" else "0")
    kc.check_long_ring(DEV, None)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 18, 40])
def test_repeat_streams_are_bit_identical(gpu_lib, B):
    kc.check_repeat_streams(DEV, None, B)


# ---- 6. snapshots and sizes; 7. API ---------------------------------------------------------------------------------------------------------
def test_state_bytes_snapshot_and_zeroed_planes(gpu_lib):
    kc.check_sizes_and_snapshot(DEV, None)


def test_api_and_refusals(gpu_lib):
    kc.check_api_and_refusals(DEV, None)
    kc.check_abi_refuses_odd_head_dim(DEV, None)


def test_batcher_on_a_4_bit_ring_equals_the_hand_driven_schedule(gpu_lib):
    kc.check_batcher(DEV, None)
