"""Per-session conditions on a real MI355X (tests/row_condition_cases.py): both head widths of k_lm_cross_attn and both batch
tiles of the per-row projection, k_cfg_mix with a coefficient per session, graph replay left untouched by a change, and the
batcher's open with a condition."""
import pytest

from tests import row_condition_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_mixed_lengths_equal_uniform_streams_bit_for_bit_tiny(gpu_lib):
    rc.check_mixed_equals_uniform(DEV, None, rc.tiny_cross_config(), [1, 15, 17, 33], steps=4)


def test_mixed_lengths_equal_uniform_streams_bit_for_bit_full_width(gpu_lib):
    rc.check_mixed_equals_uniform(DEV, None, rc.wide_cross_config(), [1, 5, 17], steps=2)


def test_mixed_lengths_equal_uniform_streams_bit_for_bit_full_width_32_row_tile(gpu_lib):
    rc.check_mixed_equals_uniform(DEV, None, rc.wide_cross_config(), [(1, 3, 4, 5, 31, 32, 33)[b % 7] for b in range(20)], steps=2, cap=33)


def test_each_session_matches_a_one_session_oracle_tiny(gpu_lib):
    rc.check_sessions_vs_oracle(DEV, None, rc.tiny_cross_config(), rc.GUIDED_COEFS, rc.GUIDED_LENGTHS, steps=4)


def test_each_session_matches_a_one_session_oracle_full_width(gpu_lib):
    rc.check_sessions_vs_oracle(DEV, None, rc.wide_cross_config(), rc.GUIDED_COEFS[:3], rc.GUIDED_LENGTHS[:3], steps=2)


def test_a_change_mid_stream_touches_one_session(gpu_lib):
    rc.check_change_mid_stream(DEV, None)


def test_a_snapshot_carries_conditions_lengths_and_coefficients(gpu_lib):
    rc.check_snapshot(DEV, None)


def test_mixed_guided_streams_repeat_bit_for_bit_full_width(gpu_lib):
    rc.check_repeat_streams(DEV, None, rc.wide_cross_config(), B=9, steps=2)


def test_refusals_raise_and_leave_the_handle_usable(gpu_lib):
    rc.check_refusals(DEV, None)


def test_batcher_channels_with_their_own_conditions(gpu_lib):
    rc.check_batcher_conditions(DEV, None)
