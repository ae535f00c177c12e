"""An LM handle of 65..128 model rows on the CPU kernel simulator (tests/many_rows_cases.py): k_gemm_rows' indexing, K partition,
reduction and epilogues, the step program above 64 rows, and the entry points."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import many_rows_cases as mr

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("ntw,ksplit", [(None, None), (2, None), (None, 2), (2, 3)])
def test_every_linear_family_equals_exact_sums(sim_lib, ntw, ksplit):
    assert mr.check_linears_exact("cpu", sim_lib, ntw=ntw, ksplit=ksplit) >= 40


@pytest.mark.parametrize("B", [65, 128])
@pytest.mark.parametrize("kind", ["moshi", "stt"])
def test_network_vs_oracle(sim_lib, kind, B):
    mr.check_network_vs_oracle("cpu", sim_lib, kind, B)


@pytest.mark.parametrize("B", [65, 128])
def test_network_vs_oracle_with_the_e4m3_kv_ring(sim_lib, B):
    mr.check_network_vs_oracle("cpu", sim_lib, "moshi", B, kv="fp8")


def test_tts_shaped_guided_sessions_with_the_script_machine_vs_the_reference_run(sim_lib):
    mr.check_tts_guided_sessions_vs_reference("cpu", sim_lib)


def test_rows_do_not_depend_on_their_tile(sim_lib):
    mr.check_rows_do_not_depend_on_their_tile("cpu", sim_lib)


def test_guided_sessions_across_the_tile_boundary_vs_one_session_oracles(sim_lib):
    mr.check_guided_sessions_vs_oracle("cpu", sim_lib)


@pytest.mark.parametrize("B", [96, 128])
def test_repeat_streams_are_bit_identical(sim_lib, B):
    mr.check_repeat_streams("cpu", sim_lib, B)


_SCHED = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests/hipsim")
import os
os.environ["MMI_NO_GRAPH"] = "1"
import build_sim
from moshi_amd import _capi
from tests import many_rows_cases as mr
mr.check_repeat_streams("cpu", _capi.load(build_sim.build()), int(sys.argv[2]), repeats=1)
print("ok")
"""


@pytest.mark.parametrize("sched", ["reverse", "random:7"])
@pytest.mark.parametrize("B", [96, 128])
def test_repeat_streams_under_other_workgroup_schedules(sim_lib, tmp_path, B, sched):
    """HIPSIM_SCHED is read when the simulator starts: a child process per schedule."""
    script = tmp_path / "sched.py"
    script.write_text(_SCHED)
    env = dict(os.environ, HIPSIM_SCHED=sched)
    p = subprocess.run([sys.executable, str(script), str(ROOT), str(B)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]


def test_snapshot_resumes_bit_for_bit_at_100_rows(sim_lib):
    mr.check_snapshot("cpu", sim_lib)


def test_batcher_of_40_guided_slots_equals_the_hand_driven_schedule(sim_lib):
    mr.check_batcher("cpu", sim_lib)


def test_refusals_and_entry_points(sim_lib):
    mr.check_refusals_and_api("cpu", sim_lib)


def test_the_row_group_control_computes_the_same_network(sim_lib):
    mr.check_control_equals_kernel("cpu", sim_lib)


def test_header_prototype_equals_the_ctypes_signature():
    import ctypes as C
    import re
    from moshi_amd import _capi
    text = (ROOT / "include" / "moshi_mi.h").read_text()
    m = re.search(r"int mmi_lm_create_rows\(([^;]*)\);", text)
    assert m, "mmi_lm_create_rows is not declared in the header"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const mmi_lm_cfg* cfg", "const mmi_lm_cfg_ext* ext_or_null", "const mmi_tensor_desc* weights", "int32_t n_weights",
                      "int32_t max_rows", "mmi_lm** out"]
    proto = next(v for k, v in vars(_capi).items() if isinstance(v, dict) and "mmi_lm_create_rows" in v)
    res, args = proto["mmi_lm_create_rows"]
    assert res is C.c_int
    assert args == [C.POINTER(_capi.LMCfg), C.POINTER(_capi.LMCfgExt), C.POINTER(_capi.TensorDesc), C.c_int32, C.c_int32,
                    C.POINTER(C.c_void_p)]
    assert proto["mmi_lm_create_rows"] == proto["mmi_lm_create_ext"]          # the same argument list, another bound


def test_server_and_cli_size_the_handle_by_rows():
    from moshi_amd.loaders import lm_size_kwargs
    assert lm_size_kwargs(64) == {"max_batch": 64} and lm_size_kwargs(32, 2) == {"max_batch": 64}
    assert lm_size_kwargs(65) == {"max_rows": 65} and lm_size_kwargs(64, 2) == {"max_rows": 128}


def test_native_selftest_rows_mode_on_the_simulator_build(sim_lib, tmp_path):
    """scripts/native_selftest.cpp --rows: a Python-free program that makes 65- and 128-row handles through mmi_lm_create_rows,
    steps them against the oracle's recorded values and resumes from a snapshot (the program a sanitizer build is made of)."""
    sys.path.insert(0, str(ROOT / "tests" / "hipsim"))
    import build_sim
    hipsim = ROOT / "tests" / "hipsim"
    exe, lib = tmp_path / "native_selftest_sim", Path(sim_lib.path)
    subprocess.check_call([build_sim._cxx(), "-O1", "-w", "-std=c++17", "-ffp-contract=off", "-pthread", "-DMMI_SELFTEST_SIM", f"-I{hipsim}",
                           f"-I{ROOT / 'include'}", str(ROOT / "scripts" / "native_selftest.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}",
                           "-o", str(exe)])
    p = subprocess.run([str(exe), str(ROOT / "tests" / "golden" / "native_selftest"), "--rows", "65,128"], capture_output=True, text=True,
                       timeout=600, env={"MMI_NO_GRAPH": "1"})
    assert p.returncode == 0 and "SELFTEST PASSED" in p.stdout, p.stdout + p.stderr
    assert "lm 65 rows" in p.stdout and "lm 128 rows" in p.stdout and p.stdout.count("0 of 3 steps differ after the snapshot") == 2
