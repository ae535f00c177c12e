"""Teacher-forced scoring on the prefill path (`mmi_lm_score`) on the CPU kernel simulator: tests/score_cases.py -
k_score_logprob alone against numpy in float64, and the call against its definition (the forced steps' parity taps, through the oracle)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import score_cases as sc
from tests.lm_cases import cached_lm_state_dict

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lm(sim_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=8, lib=sim_lib)


# ---- 1. the output kernel alone
@pytest.mark.parametrize("N", sc.WIDTHS)
def test_score_rows_equal_the_float64_log_softmax(lm, N):
    sc.check_output_kernel(lm, N)


# ---- 2. / 3. score equals forced steps, against the oracle; logp and argmax against the call's own logits
@pytest.mark.parametrize("rows", [128, 32, 5])
def test_scored_moshi_frames_are_the_oracles_steps(sim_lib, rows):
    sc.check_score_vs_oracle("cpu", sim_lib, "moshi", prefill_rows=rows)


@pytest.mark.parametrize("rows", [32, 5])
def test_scored_stt_frames_are_the_oracles_steps(sim_lib, rows):
    sc.check_score_vs_oracle("cpu", sim_lib, "stt", prefill_rows=rows)


@pytest.mark.parametrize("kv", ["fp8", "fp4"])
@pytest.mark.parametrize("rows", [128, 5])
def test_scored_frames_on_quantised_rings_are_the_oracles_steps(sim_lib, kv, rows):
    sc.check_score_vs_oracle("cpu", sim_lib, "moshi", prefill_rows=rows, kv=kv)


def test_score_with_a_sum_condition_per_session(sim_lib):
    sc.check_score_vs_oracle("cpu", sim_lib, "moshi", prefill_rows=32, cond=True)


def test_score_honours_a_depformer_weight_schedule(sim_lib):
    sc.check_score_vs_forced_steps("cpu", sim_lib, sc.schedule_config())


# ---- 4. commit = 1 is prefill
@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_commit_1_leaves_the_sessions_where_prefill_leaves_them(sim_lib, kv):
    sc.check_commit_is_prefill("cpu", sim_lib, kv=kv)


# ---- 5. commit = 0 leaves no trace
@pytest.mark.parametrize("kv", ["bf16", "fp4"])
def test_commit_0_leaves_no_trace(sim_lib, kv):
    sc.check_commit0_leaves_no_trace("cpu", sim_lib, kv=kv)


# ---- 6. / 7.
def test_score_between_steps_of_a_live_batch_leaves_the_neighbours_alone(sim_lib):
    sc.check_between_steps_of_a_live_batch("cpu", sim_lib)


def test_refusals_and_the_off_state(sim_lib):
    sc.check_refusals_and_off_state("cpu", sim_lib)


# ---- 5. again, under other workgroup schedules
_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import hashlib
import build_sim
from moshi_amd import _capi
from tests import score_cases as sc
out = sc.check_commit0_leaves_no_trace("cpu", _capi.load(build_sim.build()))
h = hashlib.sha256()
for a in out:
    h.update(a.tobytes())
print("ok", h.hexdigest())
"""


def test_the_repeated_commit_0_call_under_other_workgroup_schedules(sim_lib, tmp_path):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule.  The four outputs are the same bytes under every
    schedule (no atomics, a fixed tree)."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    digests = []
    for sched in ("reverse", "random:7"):
        env = dict(os.environ, HIPSIM_SCHED=sched)
        p = subprocess.run([sys.executable, str(script), str(ROOT)], capture_output=True, text=True, timeout=900, env=env)
        assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]
        digests.append(p.stdout.split("ok")[-1].split()[0])
    assert digests[0] == digests[1], "the outputs depend on the workgroup schedule"
