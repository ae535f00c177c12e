"""The TTS script machine on the kernel simulator (tests/tts_machine_cases.py): the device machine against the reference's
`StateMachine` and against the reference's `LMGen` under generate()-style hooks, lifecycle, launch budget and refusals."""
import pytest

from tests import tts_machine_cases as cases


def test_golden_holds_every_situation_and_the_host_restatement_equals_it():
    cases.check_golden_holds_every_situation_and_host_machine_equals_it()


@pytest.mark.parametrize("ahead", [0, 2])
def test_machine_alone_equals_the_reference_state_machine(sim_lib, ahead):
    cases.check_machine_alone("cpu", sim_lib, ahead)


def test_whole_step_equals_the_reference_run_and_the_pad_bonus_is_exact(sim_lib):
    cases.check_whole_step_against_reference("cpu", sim_lib)


def test_device_machine_equals_host_hooks_step_for_step(sim_lib):
    cases.check_device_equals_host("cpu", sim_lib)


def test_host_hooks_next_to_the_machine_run_behind_it(sim_lib):
    cases.check_host_hooks_run_behind_the_machine("cpu", sim_lib)


def test_mask_reset_snapshot_and_script_change_per_row(sim_lib):
    cases.check_lifecycle("cpu", sim_lib)


def test_launch_budget_and_machine_off_list(sim_lib):
    cases.check_launch_budget("cpu", sim_lib)


def test_refusals_change_nothing(sim_lib):
    cases.check_refusals("cpu", sim_lib)
