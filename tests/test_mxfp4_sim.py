"""OCP MXFP4 linears on the CPU: the quantiser, and the engine's 4-bit kernels (k_pack_w_fp4, k_gemm_xp / k_gemm_xp_norm WQ = 4)
on the kernel simulator, where the conversion is the plain restatement of mmi_fp4.h (tests/mxfp4_cases.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import mxfp4_cases as mx

ROOT = Path(__file__).resolve().parent.parent


def test_quantiser_on_crafted_blocks():
    mx.check_quantiser_crafted_blocks()


def test_quantise_dequantise_quantise_reproduces_the_bytes():
    mx.check_quantise_dequantise_quantise()


def test_exported_checkpoint_loads_through_from_local(sim_lib, tmp_path):
    mx.check_exporter_round_trip(sim_lib, tmp_path)


@pytest.mark.parametrize("max_batch", [16, 32])
def test_one_hot_rows_read_the_dequantised_columns(sim_lib, max_batch):
    mx.check_one_hot_columns("cpu", sim_lib, max_batch)


@pytest.mark.parametrize("ksplit", [None, 2, 3])
@pytest.mark.parametrize("max_batch", [16, 32, 64])
def test_every_linear_family_equals_exact_sums(sim_lib, max_batch, ksplit):
    assert mx.check_linears_exact("cpu", sim_lib, max_batch, ksplit=ksplit) >= 12 * len(mx.EXACT_ROWS[max_batch])


@pytest.mark.parametrize("B", [3, 40])
@pytest.mark.parametrize("kind", ["moshi", "stt"])
def test_network_vs_the_bf16_oracle_on_the_dequantised_weights(sim_lib, kind, B):
    mx.check_network_vs_oracle("cpu", sim_lib, kind, B)


@pytest.mark.parametrize("B", [3, 40])
def test_repeat_streams_are_bit_identical(sim_lib, B):
    mx.check_repeat_streams("cpu", sim_lib, B)


_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import build_sim
from moshi_amd import _capi
from tests import mxfp4_cases as mx
mx.check_repeat_streams("cpu", _capi.load(build_sim.build()), int(sys.argv[2]), repeats=1)
print("ok")
"""


@pytest.mark.parametrize("sched", ["reverse", "random:7"])
@pytest.mark.parametrize("B", [3, 40])
def test_repeat_streams_under_other_workgroup_schedules(sim_lib, tmp_path, B, sched):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    env = dict(os.environ, HIPSIM_SCHED=sched)
    p = subprocess.run([sys.executable, str(script), str(ROOT), str(B)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]


def test_refusals(sim_lib):
    mx.check_refusals("cpu", sim_lib)


def test_bf16_int8_and_fp8_handles_do_not_notice_an_mxfp4_handle(sim_lib):
    mx.check_other_classes_do_not_notice("cpu", sim_lib)
