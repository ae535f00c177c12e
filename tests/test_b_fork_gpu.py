"""Forking a live session into other slots on a real MI355X: tests/fork_cases.py through the C ABI of the product
library (k_fork_ring's 16-byte non-temporal path, the captured step graph on both sides of the copy)."""
import pytest

from tests import fork_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("d", fc.DEPTHS)
@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_copy_continues_like_its_source_and_like_the_control(gpu_lib, kv, d):
    fc.check_continuation(DEV, None, kv, d)


@pytest.mark.parametrize("d", fc.DEPTHS)
def test_seeded_draw_stream_continues_in_the_copy(gpu_lib, d):
    fc.check_continuation(DEV, None, "bf16", d, seeded=True)


def test_three_destinations_in_one_call_then_three_seeds(gpu_lib):
    fc.check_several_destinations(DEV, None)


@pytest.mark.parametrize("cross", [False, True])
def test_guided_stream_copies_both_model_rows_and_the_condition(gpu_lib, cross):
    fc.check_guided(DEV, None, cross)


@pytest.mark.parametrize("d", [1, 5])
def test_guided_stream_restored_from_a_snapshot_then_forked(gpu_lib, d):
    fc.check_guided_after_restore(DEV, None, d)


def test_copy_finishes_the_source_script(gpu_lib):
    fc.check_tts_machine(DEV, None)


def test_copy_runs_on_the_source_adapter_slot(gpu_lib):
    fc.check_adapter(DEV, None)


def test_fork_across_the_32_and_64_row_tile_boundaries(gpu_lib):
    fc.check_many_rows(DEV, None)


def test_destination_logprob_rows_are_cleared(gpu_lib):
    fc.check_logprobs(DEV, None)


@pytest.mark.parametrize("f", [0, 1, 3, 5])
def test_codec_copy_continues_like_its_source(gpu_lib, f):
    fc.check_codec(DEV, None, f)


def test_batcher_fork(gpu_lib):
    fc.check_batcher(DEV, None)


def test_refusals_change_nothing(gpu_lib):
    fc.check_refusals(DEV, None)
