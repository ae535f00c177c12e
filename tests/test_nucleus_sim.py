"""Nucleus (top-p) sampling on the CPU kernel simulator (tests/nucleus_cases.py): the rule pinned on the reference's recorded nucleus
sizes, the mass-weighted select of k_sample_nucleus on crafted and exact rows, the table behind the row table, the entry points
and what they refuse."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import nucleus_cases as nc
from tests import sampler_cases as sc

ROOT = Path(__file__).resolve().parent.parent


def test_the_float64_rule_brackets_the_references_nucleus_on_every_fixture_row(capsys):
    """DELTA = 2^-10 (nucleus_cases): the reference's sequential fp32 cumsum stayed inside the bracket on all 633 fixture rows when the
    fixture was made; on the dyadic rows the three sizes are equal."""
    n, worst = nc.check_fixture()
    with capsys.disabled():
        print(f" [{n} fixture rows, widest bracket {worst} entries] ", end="")


def test_the_two_sided_rule_regenerates_at_most_two_percent_of_the_rows(capsys):
    rate = nc.check_regeneration_rate()
    with capsys.disabled():
        print(f" [{nc.stats['rows']} rows, {100 * rate:.2f} % regenerated] ", end="")


@pytest.mark.parametrize("V", sc.VOCABS)
def test_crafted_rows_token_for_token_and_against_top_k(sim_lib, V):
    nc.check_crafted("cpu", sim_lib, V)


@pytest.mark.parametrize("V,m", nc.DYADIC_SHAPES)
def test_large_nuclei_on_exact_sums(sim_lib, V, m):
    nc.check_dyadic("cpu", sim_lib, V, m)


def test_the_window_walk_on_exact_sums(sim_lib):
    nc.check_dyadic("cpu", sim_lib, *nc.WINDOW_WALK, walk=True)


def test_a_tiny_top_p_is_the_greedy_stream(sim_lib):
    nc.check_tiny_p_is_greedy("cpu", sim_lib)


def test_top_p_zero_on_an_enabled_handle_is_todays_stream_and_the_plain_launch_list_is_the_parents(sim_lib):
    nc.check_enabled_zero_is_today("cpu", sim_lib)


def test_every_sites_token_follows_from_the_logits_taps(sim_lib):
    nc.check_taps("cpu", sim_lib)


def test_a_session_with_its_own_top_p_does_not_depend_on_its_slot(sim_lib):
    nc.check_slot_independence("cpu", sim_lib)


def test_changing_one_sessions_top_p_changes_no_other_and_a_snapshot_restores_it(sim_lib):
    nc.check_change_and_snapshot("cpu", sim_lib)


def test_guidance_addresses_sessions_not_twins(sim_lib):
    nc.check_guided_addresses_sessions("cpu", sim_lib)


def test_a_many_row_handle(sim_lib):
    nc.check_many_rows("cpu", sim_lib)


def test_refusals_raise_and_leave_the_handle_usable(sim_lib):
    nc.check_refusals("cpu", sim_lib)


def test_batcher_channels_bring_their_own_top_p(sim_lib):
    nc.check_batcher_channels("cpu", sim_lib)


def test_server_query_accepts_text_topp_and_audio_topp():
    from moshi_amd.server import parse_session_query
    s = parse_session_query({"text_topp": "0.9", "audio_topp": "0.95", "text_topk": "12"})
    assert (s.top_p_text, s.top_p, s.top_k_text) == (0.9, 0.95, 12)
    for q in ({"text_topp": "1.5"}, {"audio_topp": "-0.1"}, {"audio_topp": "nan"}, {"text_topp": "x"}):
        with pytest.raises(ValueError):
            parse_session_query(q)


def test_duplex_pipeline_with_nucleus_rows_is_bit_identical_to_the_serial_loop(sim_lib):
    nc.check_duplex("cpu", sim_lib)


def test_a_repeated_stream_is_bit_identical(sim_lib):
    nc.check_repeat("cpu", sim_lib)


_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import build_sim
from moshi_amd import _capi
from tests import nucleus_cases as nc
nc.check_repeat("cpu", _capi.load(build_sim.build()), int(sys.argv[2]), runs=2)
print("ok")
"""


@pytest.mark.parametrize("sched", ["reverse", "random:7"])
@pytest.mark.parametrize("V", [2048, 32000])
def test_a_repeated_stream_under_other_workgroup_schedules(sim_lib, tmp_path, V, sched):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule.  check_repeat also holds the tokens to the
    float64 expectation, so a schedule-dependent sum would show against the default schedule's run as well."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    env = dict(os.environ, HIPSIM_SCHED=sched)
    p = subprocess.run([sys.executable, str(script), str(ROOT), str(V)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]
