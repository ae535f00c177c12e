"""The layout of the LM engine's streaming state on a real MI355X, against the same golden file as the simulator test
(tests/state_layout_cases.py): byte counts, the regions text, the launch list and - where no GEMM runs at the start - the bytes of
the snapshot right after streaming_start.  Start-ups and three steps of tiny models."""
import pytest

from tests import state_layout_cases as sl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(sl.CONFIGS))
def test_layout_start_bytes_and_launch_list_equal_the_recorded_ones(gpu_lib, name):
    sl.check(name, "cuda", None, on_device=True)
