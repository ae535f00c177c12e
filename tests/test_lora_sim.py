"""Per-session LoRA adapters, unmerged, on the CPU kernel simulator (tests/lora_cases.py)."""
import pytest

from tests import lora_cases as lo


def test_mixed_slots_match_the_reference_unfused_golden(sim_lib):
    lo.check_golden_mixed_slots("cpu", sim_lib)


@pytest.mark.parametrize("ksplit", [None, "2", "3"])
@pytest.mark.parametrize("max_batch", [16, 32, 64])
def test_every_linear_family_on_exact_sums(sim_lib, max_batch, ksplit):
    assert lo.check_linears_exact("cpu", sim_lib, max_batch, ksplit) >= 10 * len(lo.EXACT_ROWS[max_batch])


def test_same_session_in_slot_0_and_in_the_last_slot(sim_lib):
    lo.check_slot_independence("cpu", sim_lib)


@pytest.mark.parametrize("B", [1, 3, 18, 34])
def test_rows_without_adapter_equal_a_plain_handle(sim_lib, B):
    lo.check_all_rows_without_adapter_equal_plain("cpu", sim_lib, B, steps=2)


def test_adapter_in_an_unused_slot_changes_nothing(sim_lib):
    lo.check_unused_slot_changes_nothing("cpu", sim_lib)


def test_guidance_twins_take_the_sessions_adapter(sim_lib):
    lo.check_guidance_twins_take_the_adapter("cpu", sim_lib)


@pytest.mark.parametrize("B", [3, 40])
def test_repeat_streams_are_bit_identical(sim_lib, B):
    lo.check_repeat_streams("cpu", sim_lib, B, steps=2)


def test_set_mid_stream_snapshot_reset_and_no_rebuild(sim_lib):
    lo.check_state_behaviour("cpu", sim_lib)


def test_batcher_open_and_close_set_and_clear_the_slot(sim_lib):
    lo.check_batcher_open_close("cpu", sim_lib)


def test_refusals(sim_lib):
    lo.check_refusals("cpu", sim_lib)


def test_plain_handles_do_not_notice(sim_lib):
    lo.check_other_classes_do_not_notice("cpu", sim_lib)
