"""Log-probabilities of the live step (`mmi_lm_enable_logprobs`) on the CPU kernel simulator: tests/logprob_cases.py -
k_step_logprob alone against numpy in float64 and bit for bit against k_score_logprob, the op inside the step against the tap on the
step's own logits, the read-outs, the batcher and the refusals."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from moshi_amd import LMModel
from moshi_amd.config import LMConfig, tiny_lm_config
from tests import logprob_cases as lc
from tests.lm_cases import cached_lm_state_dict

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lm(sim_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=8, lib=sim_lib)


# ---- A. the kernel alone
@pytest.mark.parametrize("N", lc.WIDTHS)
def test_the_kernel_alone_equals_float64_and_the_scoring_kernel(lm, N):
    lc.check_kernel(lm, N)


_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import hashlib
import build_sim
from moshi_amd import LMModel, _capi
from moshi_amd.config import tiny_lm_config
from tests import logprob_cases as lc
from tests.lm_cases import cached_lm_state_dict
cfg = tiny_lm_config()
lm = LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=8, lib=_capi.load(build_sim.build()))
print("ok", hashlib.sha256(lc.tie_digest(lm)).hexdigest())
"""


def test_the_ties_under_other_workgroup_schedules(lm, tmp_path):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule.  The tie cases give the same bytes under every
    schedule (a fixed tree, no atomics)."""
    import hashlib
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    digests = [hashlib.sha256(lc.tie_digest(lm)).hexdigest()]
    for sched in ("reverse", "random:7"):
        env = dict(os.environ, HIPSIM_SCHED=sched)
        p = subprocess.run([sys.executable, str(script), str(ROOT)], capture_output=True, text=True, timeout=900, env=env)
        assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]
        digests.append(p.stdout.split("ok")[-1].split()[0])
    assert len(set(digests)) == 1, "the outputs depend on the workgroup schedule"


# ---- B. in the step
@pytest.mark.parametrize("top_n", [0, 3, 8])
def test_both_read_outs_after_every_step_under_a_mask_and_a_reset(sim_lib, top_n):
    lc.check_in_step("cpu", sim_lib, top_n=top_n)


def test_both_read_outs_at_the_full_vocabularies(sim_lib):
    lc.check_in_step("cpu", sim_lib, LMConfig(num_layers=1, context=16), n=2, steps=3, top_n=8)


# ---- C. forcing and hooks
def test_a_forced_initial_token_and_a_replaced_text_token(sim_lib):
    lc.check_forcing_and_hooks("cpu", sim_lib)


# ---- D. other handles
@pytest.mark.parametrize("no_text", [False, True])
def test_a_guided_stream(sim_lib, no_text):
    lc.check_guided("cpu", sim_lib, no_text)


@pytest.mark.parametrize("kind", ["int8", "kv_fp4", "rows96", "stt"])
def test_other_handles(sim_lib, kind):
    lc.check_other_handle("cpu", sim_lib, kind)


def test_a_tts_machine_stream(sim_lib):
    lc.check_tts_machine("cpu", sim_lib)


# ---- E. / F. / G.
def test_the_off_state_and_a_repeated_stream(sim_lib):
    lc.check_off_state_and_repeat("cpu", sim_lib)


def test_the_batcher_queues_each_frames_values(sim_lib):
    lc.check_batcher("cpu", sim_lib)


def test_refusals(sim_lib):
    lc.check_refusals("cpu", sim_lib)
