"""Per-session sampling on the CPU kernel simulator (tests/row_sampling_cases.py): the table read in k_sample, the per-row draw
counter, the two logit adjustments, the ring k_lm_commit keeps, the entry points and what they refuse."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import row_sampling_cases as rc
from tests import sampler_cases as sc

ROOT = Path(__file__).resolve().parent.parent


def test_the_tie_rule_refuses_at_most_two_percent_of_the_mixed_rows(capsys):
    rate = rc.check_mixed_drop_rate()
    with capsys.disabled():
        print(f" [tie rule: {100 * rate:.2f} % of the mixed rows regenerated] ", end="")


@pytest.mark.parametrize("V", sc.VOCABS)
def test_mixed_rows_match_the_float64_reference_token_for_token(sim_lib, V):
    rc.check_mixed_rows("cpu", sim_lib, V)


@pytest.mark.parametrize("V", [1000, 32000])
def test_sessions_do_not_depend_on_their_slot_crafted(sim_lib, V):
    rc.check_slot_independence("cpu", sim_lib, V)


def test_inactive_rows_do_depend_on_their_slot(sim_lib):
    rc.check_slot_independence("cpu", sim_lib, 1000, active=False)


def test_sessions_do_not_depend_on_their_slot_free_running(sim_lib):
    from moshi_amd.config import tiny_lm_config
    rc.check_slot_independence("cpu", sim_lib, tiny_lm_config().text_card, crafted=False, steps=12)


def test_one_session_equals_a_one_session_lmgen_of_today(sim_lib):
    rc.check_equals_one_session_lmgen("cpu", sim_lib)


@pytest.mark.parametrize("V,steps", [(1000, 70), (8192, 14), (32000, 14)])
def test_repetition_penalty_and_pad_bias_follow_the_restated_rules(sim_lib, V, steps):
    rc.check_penalty_and_pad("cpu", sim_lib, V, steps=steps)


def test_lifecycle_set_reset_clear_snapshot(sim_lib):
    rc.check_lifecycle("cpu", sim_lib)


def test_guidance_addresses_sessions_not_twins(sim_lib):
    rc.check_guided_addresses_sessions("cpu", sim_lib)


def test_refusals_raise_and_leave_the_handle_usable(sim_lib):
    rc.check_refusals("cpu", sim_lib)


def test_the_ring_skips_the_models_own_end_of_padding_id(sim_lib):
    rc.check_end_padding_id_of_the_model("cpu", sim_lib)


def test_duplex_pipeline_with_active_rows_is_bit_identical_to_the_serial_loop(sim_lib):
    rc.check_duplex_with_active_rows("cpu", sim_lib)


@pytest.mark.parametrize("V", [2048, 32000])
def test_mixed_rows_repeat_bit_for_bit_on_fresh_streams(sim_lib, V):
    rc.check_repeat_streams("cpu", sim_lib, V)


_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import build_sim
from moshi_amd import _capi
from tests import row_sampling_cases as rc
rc.check_repeat_streams("cpu", _capi.load(build_sim.build()), int(sys.argv[2]))
print("ok")
"""


@pytest.mark.parametrize("sched", ["reverse", "random:7"])
@pytest.mark.parametrize("V", [2048, 32000])
def test_mixed_rows_repeat_under_other_workgroup_schedules(sim_lib, tmp_path, V, sched):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    env = dict(os.environ, HIPSIM_SCHED=sched)
    p = subprocess.run([sys.executable, str(script), str(ROOT), str(V)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]


def test_row_sampling_struct_layout_of_the_header_equals_the_binding(tmp_path):
    """mmi_row_sampling is declared like mmi_lm_cfg_ext (struct + typedef), next to the structs test_capi.py lays out."""
    import ctypes
    from moshi_amd import _capi
    fields = [n for n, _ in _capi.RowSampling._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "moshi_mi.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(mmi_row_sampling));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mmi_row_sampling, {f}));' for f in fields] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "layout")])
    for ln in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        f, v = ln.split()
        if f == ".":
            assert ctypes.sizeof(_capi.RowSampling) == int(v)
        else:
            assert getattr(_capi.RowSampling, f).offset == int(v), f
