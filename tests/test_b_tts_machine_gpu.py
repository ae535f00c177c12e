"""The TTS script machine on the MI355X (tests/tts_machine_cases.py), with the step captured as a graph."""
import pytest

from tests import tts_machine_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ahead", [0, 2])
def test_machine_alone_equals_the_reference_state_machine(gpu_lib, ahead):
    cases.check_machine_alone("cuda", gpu_lib, ahead)


def test_whole_step_equals_the_reference_run_and_the_pad_bonus_is_exact(gpu_lib):
    cases.check_whole_step_against_reference("cuda", gpu_lib)


def test_device_machine_equals_host_hooks_step_for_step(gpu_lib):
    cases.check_device_equals_host("cuda", gpu_lib)


def test_host_hooks_next_to_the_machine_run_behind_it(gpu_lib):
    cases.check_host_hooks_run_behind_the_machine("cuda", gpu_lib)


def test_mask_reset_snapshot_and_script_change_per_row(gpu_lib):
    cases.check_lifecycle("cuda", gpu_lib)


def test_machine_on_step_is_bit_identical_eager_and_graphed(gpu_lib):
    cases.check_eager_equals_graphed("cuda", gpu_lib)


def test_launch_budget_and_machine_off_list(gpu_lib):
    cases.check_launch_budget("cuda", gpu_lib)


def test_refusals_change_nothing(gpu_lib):
    cases.check_refusals("cuda", gpu_lib)
