"""Per-session LoRA adapters, unmerged, on the MI355X (tests/lora_cases.py): the LORA / shrink forms of k_gemm_xp on the matrix
cores, the step captured as a graph, and one 7B layer's widths."""
import pytest

from tests import lora_cases as lo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_mixed_slots_match_the_reference_unfused_golden(gpu_lib):
    lo.check_golden_mixed_slots(DEV, gpu_lib)


@pytest.mark.parametrize("ksplit", [None, "2", "3"])
@pytest.mark.parametrize("max_batch", [16, 32, 64])
def test_every_linear_family_on_exact_sums(gpu_lib, max_batch, ksplit):
    assert lo.check_linears_exact(DEV, gpu_lib, max_batch, ksplit) >= 10 * len(lo.EXACT_ROWS[max_batch])


def test_one_7b_layer_widths_on_exact_sums(gpu_lib):
    lo.check_7b_layer_shapes(DEV, gpu_lib)


def test_same_session_in_slot_0_and_in_the_last_slot(gpu_lib):
    lo.check_slot_independence(DEV, gpu_lib)


@pytest.mark.parametrize("B", [1, 3, 18, 34])
def test_rows_without_adapter_equal_a_plain_handle(gpu_lib, B):
    lo.check_all_rows_without_adapter_equal_plain(DEV, gpu_lib, B)


def test_adapter_in_an_unused_slot_changes_nothing(gpu_lib):
    lo.check_unused_slot_changes_nothing(DEV, gpu_lib)


def test_guidance_twins_take_the_sessions_adapter(gpu_lib):
    lo.check_guidance_twins_take_the_adapter(DEV, gpu_lib)


@pytest.mark.parametrize("B", [3, 40])
def test_repeat_streams_are_bit_identical(gpu_lib, B):
    lo.check_repeat_streams(DEV, gpu_lib, B)


def test_set_mid_stream_snapshot_reset_and_no_rebuild(gpu_lib):
    lo.check_state_behaviour(DEV, gpu_lib)


def test_batcher_open_and_close_set_and_clear_the_slot(gpu_lib):
    lo.check_batcher_open_close(DEV, gpu_lib)


def test_refusals(gpu_lib):
    lo.check_refusals(DEV, gpu_lib)


def test_plain_handles_do_not_notice(gpu_lib):
    lo.check_other_classes_do_not_notice(DEV, gpu_lib)
