"""Chunked prefill (`mmi_lm_prefill`) on the MI355X: the cases of tests/test_prefill_sim.py (tests/prefill_cases.py) with
what the simulator never runs - v_mfma_f32_32x32x16_bf16 and v_mfma_f32_32x32x2f32 in k_lm_attn_prefill, the hardware's e4m3 and E2M1
conversions in k_pf_rope_kv - and one temporal layer at the production width."""
import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import prefill_cases as pc
from tests.lm_cases import cached_lm_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm(gpu_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=8, lib=gpu_lib)


@pytest.mark.parametrize("form,Dh", pc.ATTN_GRID)
def test_prefill_attention_equals_the_fp64_softmax(lm, form, Dh):
    pc.check_attention(lm, form, Dh)


@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_one_session_equals_forced_steps(gpu_lib, kv):
    pc.check_rings_and_state("cuda", gpu_lib, kv=kv, starts=(0,))


@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_four_sessions_at_different_offsets_equal_forced_steps(gpu_lib, kv):
    stats = {}
    pc.check_rings_and_state("cuda", gpu_lib, kv=kv, starts=(0, 5, 11, 30), active=2, stats=stats)
    assert stats["rows_launches"][0] > 0 and stats["rows_launches"][1] > 0


@pytest.mark.parametrize("T", [1, 11, 12, 37])
@pytest.mark.parametrize("rows", [128, 8])
def test_prefilled_moshi_steps_on_like_the_oracle(gpu_lib, T, rows):
    pc.check_network_vs_oracle("cuda", gpu_lib, "moshi", T=T, prefill_rows=rows)


@pytest.mark.parametrize("T", [1, 11, 12, 37])
def test_prefilled_stt_steps_on_like_the_oracle(gpu_lib, T):
    pc.check_network_vs_oracle("cuda", gpu_lib, "stt", T=T, prefill_rows=8)


@pytest.mark.parametrize("kv", ["fp8", "fp4"])
@pytest.mark.parametrize("T", [11, 37])
def test_prefilled_quantised_rings_step_on_like_the_oracle(gpu_lib, kv, T):
    pc.check_network_vs_oracle("cuda", gpu_lib, "moshi", T=T, prefill_rows=8 if T == 37 else 128, kv=kv)


def test_prefill_with_a_sum_condition_per_session(gpu_lib):
    pc.check_network_vs_oracle("cuda", gpu_lib, "moshi", T=12, prefill_rows=128, cond=True)


def test_prefill_between_steps_of_a_live_batch_leaves_the_neighbours_alone(gpu_lib):
    pc.check_between_steps_of_a_live_batch("cuda", gpu_lib)


def test_chunking_does_not_matter(gpu_lib):
    pc.check_chunking("cuda", gpu_lib)


def test_refusals_and_the_off_state(gpu_lib):
    pc.check_refusals_and_off_state("cuda", gpu_lib)


def test_a_log_of_last_tokens_rebuilds_the_session(gpu_lib):
    pc.check_last_tokens_log("cuda", gpu_lib)


@pytest.mark.parametrize("n,T", [(1, 128), (4, 32)])
@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_one_layer_at_the_production_width(gpu_lib, kv, n, T):
    pc.check_production_width("cuda", gpu_lib, kv, n, T)
