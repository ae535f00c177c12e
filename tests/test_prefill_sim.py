"""Chunked prefill (`mmi_lm_prefill`) on the CPU kernel simulator: tests/prefill_cases.py - k_lm_attn_prefill alone
against the fp64 softmax, and the call against its definition (forced steps under an exec mask of exactly the named sessions)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import prefill_cases as pc
from tests.lm_cases import cached_lm_state_dict

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lm(sim_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=8, lib=sim_lib)


# ---- 1. the attention alone
@pytest.mark.parametrize("form,Dh", pc.ATTN_GRID)
def test_prefill_attention_equals_the_fp64_softmax(lm, form, Dh):
    pc.check_attention(lm, form, Dh)


def test_the_recorded_gamma_is_what_the_case_list_gives():
    """A check of the CASE LIST, not of the kernel (numpy only): GAMMA re-measured the way DESIGN.md 8.19 measured it (fp32_twin over
    every tolerance launch) equals the figure recorded in prefill_cases, and lies below the decode kernels' constant."""
    worst, where = pc.measure_gamma(verbose=False)
    assert abs(4 * worst - pc.GAMMA_MEASURED) < 0.1 and 4 * worst <= pc.ac.GAMMA, (worst, where)


# ---- 2. / 3. layer-0 rings and every other state region, bit for bit
@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_one_session_equals_forced_steps(sim_lib, kv):
    pc.check_rings_and_state("cpu", sim_lib, kv=kv, starts=(0,))


@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_four_sessions_at_different_offsets_equal_forced_steps(sim_lib, kv):
    stats = {}
    pc.check_rings_and_state("cpu", sim_lib, kv=kv, starts=(0, 5, 11, 30), active=2, stats=stats)
    assert stats["rows_launches"][0] > 0 and stats["rows_launches"][1] > 0          # both sides ran k_gemm_rows


# ---- 4. the network against the oracle
@pytest.mark.parametrize("T", [1, 11, 12, 37])
@pytest.mark.parametrize("rows", [128, 8])
def test_prefilled_moshi_steps_on_like_the_oracle(sim_lib, T, rows):
    pc.check_network_vs_oracle("cpu", sim_lib, "moshi", T=T, prefill_rows=rows)


@pytest.mark.parametrize("T", [1, 11, 12, 37])
def test_prefilled_stt_steps_on_like_the_oracle(sim_lib, T):
    pc.check_network_vs_oracle("cpu", sim_lib, "stt", T=T, prefill_rows=8)


@pytest.mark.parametrize("kv", ["fp8", "fp4"])
@pytest.mark.parametrize("T", [11, 37])
def test_prefilled_quantised_rings_step_on_like_the_oracle(sim_lib, kv, T):
    pc.check_network_vs_oracle("cpu", sim_lib, "moshi", T=T, prefill_rows=8 if T == 37 else 128, kv=kv)


def test_prefill_with_a_sum_condition_per_session(sim_lib):
    pc.check_network_vs_oracle("cpu", sim_lib, "moshi", T=12, prefill_rows=128, cond=True)


# ---- 5. .. 8.
def test_prefill_between_steps_of_a_live_batch_leaves_the_neighbours_alone(sim_lib):
    pc.check_between_steps_of_a_live_batch("cpu", sim_lib)


def test_chunking_does_not_matter(sim_lib):
    pc.check_chunking("cpu", sim_lib)


def test_refusals_and_the_off_state(sim_lib):
    pc.check_refusals_and_off_state("cpu", sim_lib)


def test_a_log_of_last_tokens_rebuilds_the_session(sim_lib):
    pc.check_last_tokens_log("cpu", sim_lib)


# ---- 10. other workgroup schedules
_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import build_sim
from moshi_amd import _capi
from tests import prefill_cases as pc
pc.check_rings_and_state("cpu", _capi.load(build_sim.build()), kv="bf16", starts=(0, 5, 11, 30), active=2)
print("ok")
"""


@pytest.mark.parametrize("sched", ["reverse", "random:7"])
def test_rings_and_state_under_other_workgroup_schedules(sim_lib, tmp_path, sched):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    env = dict(os.environ, HIPSIM_SCHED=sched)
    p = subprocess.run([sys.executable, str(script), str(ROOT)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]
