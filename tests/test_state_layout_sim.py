"""The layout of the LM engine's streaming state on the CPU kernel simulator (tests/state_layout_cases.py): the arena's order and
sizes, which buffers streaming_start initialises and with what, the state after three steps and the launch list - each equal to
what the commit before the state table recorded (tests/golden/lm_state_layout.json)."""
import pytest

from tests import state_layout_cases as sl


def test_every_configuration_is_recorded():
    assert set(sl.load_golden()) == set(sl.CONFIGS)


@pytest.mark.parametrize("name", list(sl.CONFIGS))
def test_layout_start_bytes_steps_and_launch_list_equal_the_recorded_ones(sim_lib, name):
    sl.check(name, "cpu", sim_lib)
