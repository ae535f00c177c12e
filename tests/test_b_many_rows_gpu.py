"""An LM handle of 65..128 model rows on the MI355X (tests/many_rows_cases.py): k_gemm_rows on the matrix cores, the step above 64
rows captured as a graph."""
import pytest

from tests import many_rows_cases as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("ntw,ksplit", [(None, None), (2, None), (None, 2), (2, 3)])
def test_every_linear_family_equals_exact_sums(gpu_lib, ntw, ksplit):
    assert mr.check_linears_exact(DEV, gpu_lib, ntw=ntw, ksplit=ksplit) >= 40


@pytest.mark.parametrize("B", [65, 128])
@pytest.mark.parametrize("kind", ["moshi", "stt"])
def test_network_vs_oracle(gpu_lib, kind, B):
    mr.check_network_vs_oracle(DEV, gpu_lib, kind, B)


@pytest.mark.parametrize("B", [65, 128])
def test_network_vs_oracle_with_the_e4m3_kv_ring(gpu_lib, B):
    mr.check_network_vs_oracle(DEV, gpu_lib, "moshi", B, kv="fp8")


def test_tts_shaped_guided_sessions_with_the_script_machine_vs_the_reference_run(gpu_lib):
    mr.check_tts_guided_sessions_vs_reference(DEV, gpu_lib)


def test_rows_do_not_depend_on_their_tile(gpu_lib):
    mr.check_rows_do_not_depend_on_their_tile(DEV, gpu_lib)


def test_guided_sessions_across_the_tile_boundary_vs_one_session_oracles(gpu_lib):
    mr.check_guided_sessions_vs_oracle(DEV, gpu_lib)


@pytest.mark.parametrize("B", [96, 128])
def test_repeat_streams_are_bit_identical(gpu_lib, B):
    mr.check_repeat_streams(DEV, gpu_lib, B, repeats=4)


def test_snapshot_resumes_bit_for_bit_at_100_rows(gpu_lib):
    mr.check_snapshot(DEV, gpu_lib)


def test_batcher_of_40_guided_slots_equals_the_hand_driven_schedule(gpu_lib):
    mr.check_batcher(DEV, gpu_lib)


def test_refusals_and_entry_points(gpu_lib):
    mr.check_refusals_and_api(DEV, gpu_lib)


def test_the_row_group_control_computes_the_same_network(gpu_lib):
    mr.check_control_equals_kernel(DEV, gpu_lib)
