"""Teacher-forced scoring on the prefill path (`mmi_lm_score`) on the MI355X: the cases of tests/test_score_sim.py
(tests/score_cases.py) with what the simulator never runs - the device expf / logf of k_score_logprob, the MFMA linears of the depth
transformer at up to 128 rows - and the shapes the tiny models do not reach: heads of 32000 and 2048 entries, a depth transformer
of width 1024 on k_gemm_rows, and the last temporal layer at the production width feeding the heads."""
import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import prefill_cases as pc
from tests import score_cases as sc
from tests.lm_cases import cached_lm_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm(gpu_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=8, lib=gpu_lib)


@pytest.mark.parametrize("N", sc.WIDTHS)
def test_score_rows_equal_the_float64_log_softmax(lm, N):
    sc.check_output_kernel(lm, N)


@pytest.mark.parametrize("rows", [128, 32, 5])
def test_scored_moshi_frames_are_the_oracles_steps(gpu_lib, rows):
    sc.check_score_vs_oracle("cuda", gpu_lib, "moshi", prefill_rows=rows)


@pytest.mark.parametrize("rows", [32, 5])
def test_scored_stt_frames_are_the_oracles_steps(gpu_lib, rows):
    sc.check_score_vs_oracle("cuda", gpu_lib, "stt", prefill_rows=rows)


@pytest.mark.parametrize("kv", ["fp8", "fp4"])
@pytest.mark.parametrize("rows", [128, 5])
def test_scored_frames_on_quantised_rings_are_the_oracles_steps(gpu_lib, kv, rows):
    sc.check_score_vs_oracle("cuda", gpu_lib, "moshi", prefill_rows=rows, kv=kv)


def test_score_with_a_sum_condition_per_session(gpu_lib):
    sc.check_score_vs_oracle("cuda", gpu_lib, "moshi", prefill_rows=32, cond=True)


def test_score_honours_a_depformer_weight_schedule(gpu_lib):
    sc.check_score_vs_forced_steps("cuda", gpu_lib, sc.schedule_config())


@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_commit_1_leaves_the_sessions_where_prefill_leaves_them(gpu_lib, kv):
    sc.check_commit_is_prefill("cuda", gpu_lib, kv=kv)


@pytest.mark.parametrize("kv", ["bf16", "fp4"])
def test_commit_0_leaves_no_trace(gpu_lib, kv):
    sc.check_commit0_leaves_no_trace("cuda", gpu_lib, kv=kv)


def test_score_between_steps_of_a_live_batch_leaves_the_neighbours_alone(gpu_lib):
    sc.check_between_steps_of_a_live_batch("cuda", gpu_lib)


def test_refusals_and_the_off_state(gpu_lib):
    sc.check_refusals_and_off_state("cuda", gpu_lib)


# ---- 8. the shapes the tiny models do not reach
def test_head_widths_and_the_depth_transformer_on_the_many_row_gemm(gpu_lib):
    """4 sessions x 32 frames = 128 rows in one pass: k_gemm_rows on every linear of a depth transformer of width 1024,
    k_score_logprob at N = 32000 and 2048."""
    sc.check_score_vs_oracle("cuda", gpu_lib, "moshi", prefill_rows=128, cfg=sc.head_width_config(), B=4, starts=(0, 9, 30, 2), T=32, rows=128,
                             want_rows_gemm=True)


def test_the_last_layer_at_the_production_width_feeds_the_heads(gpu_lib):
    """4 x 32 rows through one temporal layer of dim 4096: the last layer's attention, out_proj and FFN - which a prefill pass skips -
    feed the heads."""
    sc.check_score_vs_oracle("cuda", gpu_lib, "moshi", prefill_rows=128, cfg=pc.wide_layer_config(), B=4, starts=(0, 9, 70, 2), T=32, rows=128,
                             want_rows_gemm=True)
