"""Per-session sampling on a real MI355X (tests/row_sampling_cases.py): the three k_sample instantiations with the table, the
hardware logarithm and division, graph replay left untouched by a change of settings, and the batcher's open_with.  Tiny models,
one engine per vocabulary."""
import pytest

from tests import row_sampling_cases as rc
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("V", sc.VOCABS)
def test_mixed_rows_match_the_float64_reference_token_for_token(gpu_lib, V):
    rc.check_mixed_rows(DEV, None, V)


@pytest.mark.parametrize("V", [2048, 32000])
def test_mixed_rows_repeat_bit_for_bit_on_fresh_streams(gpu_lib, V):
    rc.check_repeat_streams(DEV, None, V)


@pytest.mark.parametrize("V", [32000, 8192, 1000])
def test_repetition_penalty_and_pad_bias_follow_the_restated_rules(gpu_lib, V):
    rc.check_penalty_and_pad(DEV, None, V, steps=70)


def test_sessions_do_not_depend_on_their_slot_crafted(gpu_lib):
    rc.check_slot_independence(DEV, None, 1000)


def test_inactive_rows_do_depend_on_their_slot(gpu_lib):
    rc.check_slot_independence(DEV, None, 1000, active=False)


def test_lifecycle_set_reset_clear_snapshot(gpu_lib):
    rc.check_lifecycle(DEV, None)


def test_guidance_addresses_sessions_not_twins(gpu_lib):
    rc.check_guided_addresses_sessions(DEV, None)


def test_refusals_raise_and_leave_the_handle_usable(gpu_lib):
    rc.check_refusals(DEV, None)


def test_sessions_do_not_depend_on_their_slot_free_running(gpu_lib):
    from moshi_amd.config import tiny_lm_config
    rc.check_slot_independence(DEV, None, tiny_lm_config().text_card, crafted=False, steps=12)


def test_one_session_equals_a_one_session_lmgen_of_today(gpu_lib):
    rc.check_equals_one_session_lmgen(DEV, None)


def test_the_ring_skips_the_models_own_end_of_padding_id(gpu_lib):
    rc.check_end_padding_id_of_the_model(DEV, None)


def test_duplex_pipeline_with_active_rows_is_bit_identical_to_the_serial_loop(gpu_lib):
    rc.check_duplex_with_active_rows(DEV, None)


def test_batcher_channels_with_their_own_settings(gpu_lib):
    rc.check_batcher_channels(DEV, None)
