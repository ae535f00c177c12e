"""Nucleus (top-p) sampling on a real MI355X (tests/nucleus_cases.py): the three k_sample_nucleus instantiations token for token on
crafted rows and on exact sums, with the hardware's logarithm and butterfly, and the properties of the table behind the row
table on free-running models."""
import pytest

from moshi_amd.config import LMConfig
from tests import nucleus_cases as nc
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("V", sc.VOCABS)
def test_crafted_rows_token_for_token_and_against_top_k(gpu_lib, V):
    nc.check_crafted(DEV, None, V)


@pytest.mark.parametrize("V,m", nc.DYADIC_SHAPES)
def test_large_nuclei_on_exact_sums(gpu_lib, V, m):
    nc.check_dyadic(DEV, None, V, m)


def test_the_window_walk_on_exact_sums(gpu_lib):
    nc.check_dyadic(DEV, None, *nc.WINDOW_WALK, walk=True)


def test_a_tiny_top_p_is_the_greedy_stream_tiny(gpu_lib):
    nc.check_tiny_p_is_greedy(DEV, None)


def test_a_tiny_top_p_is_the_greedy_stream_full_vocabularies(gpu_lib):
    """32000 text / 2048 audio entries: k_sample_nucleus<1024, 32> and <256, 8> with the fused next-input write."""
    nc.check_tiny_p_is_greedy(DEV, None, LMConfig(num_layers=1, context=16))


def test_top_p_zero_on_an_enabled_handle_is_todays_stream_and_the_plain_launch_list_is_the_parents(gpu_lib):
    nc.check_enabled_zero_is_today(DEV, None)


def test_every_sites_token_follows_from_the_logits_taps(gpu_lib):
    nc.check_taps(DEV, None)


def test_a_session_with_its_own_top_p_does_not_depend_on_its_slot(gpu_lib):
    nc.check_slot_independence(DEV, None)


def test_changing_one_sessions_top_p_changes_no_other_and_a_snapshot_restores_it(gpu_lib):
    nc.check_change_and_snapshot(DEV, None)


def test_guidance_addresses_sessions_not_twins(gpu_lib):
    nc.check_guided_addresses_sessions(DEV, None)


def test_a_many_row_handle(gpu_lib):
    nc.check_many_rows(DEV, None)


def test_refusals_raise_and_leave_the_handle_usable(gpu_lib):
    nc.check_refusals(DEV, None)


def test_batcher_channels_bring_their_own_top_p(gpu_lib):
    nc.check_batcher_channels(DEV, None)


def test_a_repeated_stream_is_bit_identical(gpu_lib):
    nc.check_repeat(DEV, None)
