"""Log-probabilities of the live step (`mmi_lm_enable_logprobs`) on the MI355X: the cases of tests/test_logprobs_sim.py
(tests/logprob_cases.py) with what the simulator never runs - the device expf / logf of k_step_logprob against k_score_logprob's, the
captured step with the extra op, the MFMA linears behind the logits - at the production head widths."""
import pytest

from moshi_amd import LMModel
from moshi_amd.config import LMConfig, tiny_lm_config
from tests import logprob_cases as lc
from tests.lm_cases import cached_lm_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm(gpu_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=8, lib=gpu_lib)


@pytest.mark.parametrize("N", [2048, 32000, 32768])
def test_the_kernel_alone_equals_float64_and_the_scoring_kernel(lm, N):
    lc.check_kernel(lm, N)


@pytest.mark.parametrize("top_n", [0, 8])
def test_both_read_outs_after_every_step_under_a_mask_and_a_reset(gpu_lib, top_n):
    lc.check_in_step("cuda", gpu_lib, top_n=top_n)


def test_both_read_outs_at_the_full_vocabularies(gpu_lib):
    lc.check_in_step("cuda", gpu_lib, LMConfig(num_layers=1, context=16), n=2, steps=3, top_n=8)


@pytest.mark.parametrize("no_text", [False, True])
def test_a_guided_stream(gpu_lib, no_text):
    lc.check_guided("cuda", gpu_lib, no_text)


def test_an_int8_handle(gpu_lib):
    lc.check_other_handle("cuda", gpu_lib, "int8")


def test_the_off_state_and_a_repeated_stream(gpu_lib):
    lc.check_off_state_and_repeat("cuda", gpu_lib)


def test_the_batcher_queues_each_frames_values(gpu_lib):
    lc.check_batcher("cuda", gpu_lib)
