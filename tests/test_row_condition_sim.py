"""Per-session conditions on the CPU kernel simulator (tests/row_condition_cases.py): the length per model row in
k_lm_cross_attn, the coefficient per session in k_cfg_mix, the per-row projection, the entry points and what they refuse."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import row_condition_cases as rc

ROOT = Path(__file__).resolve().parent.parent


def test_mixed_lengths_equal_uniform_streams_bit_for_bit(sim_lib):
    rc.check_mixed_equals_uniform("cpu", sim_lib, rc.tiny_cross_config(), [1, 15, 17, 33], steps=4)


def test_each_session_matches_a_one_session_oracle(sim_lib):
    rc.check_sessions_vs_oracle("cpu", sim_lib, rc.tiny_cross_config(), rc.GUIDED_COEFS, rc.GUIDED_LENGTHS, steps=4)


def test_a_change_mid_stream_touches_one_session(sim_lib):
    rc.check_change_mid_stream("cpu", sim_lib)


def test_a_snapshot_carries_conditions_lengths_and_coefficients(sim_lib):
    rc.check_snapshot("cpu", sim_lib)


def test_mixed_guided_streams_repeat_bit_for_bit(sim_lib):
    rc.check_repeat_streams("cpu", sim_lib)


_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import build_sim
from moshi_amd import _capi
from tests import row_condition_cases as rc
rc.check_repeat_streams("cpu", _capi.load(build_sim.build()))
print("ok")
"""


@pytest.mark.parametrize("sched", ["reverse", "random:7"])
def test_mixed_guided_streams_repeat_under_other_workgroup_schedules(sim_lib, tmp_path, sched):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    env = dict(os.environ, HIPSIM_SCHED=sched)
    p = subprocess.run([sys.executable, str(script), str(ROOT)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]


def test_refusals_raise_and_leave_the_handle_usable(sim_lib):
    rc.check_refusals("cpu", sim_lib)


def test_batcher_channels_with_their_own_conditions(sim_lib):
    rc.check_batcher_conditions("cpu", sim_lib)


def test_condition_struct_layouts_of_the_header_equal_the_binding(tmp_path):
    rc.check_layout(tmp_path, ROOT)
