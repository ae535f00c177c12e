"""scripts/native_selftest.cpp --prefill, built against the CPU simulator like tests/test_native_selftest.py builds the other modes:
chunked prefill through the C ABI alone - the recorded forced frames enter the sessions by mmi_lm_prefill, the following steps are held
to the oracle's record, and the entry points' refusal codes hold."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HIPSIM = ROOT / "tests" / "hipsim"
FIXTURE = ROOT / "tests" / "golden" / "native_selftest"


def test_native_selftest_prefill_mode_passes_on_the_simulator_build(sim_lib, tmp_path):
    sys.path.insert(0, str(HIPSIM))
    import build_sim
    exe = tmp_path / "native_selftest_sim"
    lib = Path(sim_lib.path)
    subprocess.check_call([build_sim._cxx(), "-O1", "-w", "-std=c++17", "-ffp-contract=off", "-pthread", "-DMMI_SELFTEST_SIM", f"-I{HIPSIM}",
                           f"-I{ROOT / 'include'}", str(ROOT / "scripts" / "native_selftest.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}",
                           "-o", str(exe)])
    p = subprocess.run([str(exe), str(FIXTURE), "--prefill"], capture_output=True, text=True, timeout=600, env={"MMI_NO_GRAPH": "1"})
    assert p.returncode == 0 and "SELFTEST PASSED" in p.stdout, p.stdout + p.stderr
    assert p.stdout.count("last_tokens differ in 0 entries") == 3 and p.stdout.count("steps differ from the oracle (must be 0)") == 3, p.stdout
    assert "66 sessions, 128 rows per pass" in p.stdout and "(0 k_gemm_rows launches)" in p.stdout.split("66 sessions")[0], p.stdout
    assert "8 of 8 refusal checks held" in p.stdout, p.stdout
