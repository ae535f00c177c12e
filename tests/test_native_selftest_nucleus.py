"""scripts/native_selftest.cpp --nucleus, built against the CPU simulator like tests/test_native_selftest.py builds the other modes:
the nucleus samplers through the C ABI alone - a sampling stream with top_p = top_p_text = 1e-6 equals the greedy stream of the same
tiny model, and the entry points' refusal codes hold."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HIPSIM = ROOT / "tests" / "hipsim"
FIXTURE = ROOT / "tests" / "golden" / "native_selftest"


def test_native_selftest_nucleus_mode_passes_on_the_simulator_build(sim_lib, tmp_path):
    sys.path.insert(0, str(HIPSIM))
    import build_sim
    exe = tmp_path / "native_selftest_sim"
    lib = Path(sim_lib.path)
    subprocess.check_call([build_sim._cxx(), "-O1", "-w", "-std=c++17", "-ffp-contract=off", "-pthread", "-DMMI_SELFTEST_SIM", f"-I{HIPSIM}",
                           f"-I{ROOT / 'include'}", str(ROOT / "scripts" / "native_selftest.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}",
                           "-o", str(exe)])
    p = subprocess.run([str(exe), str(FIXTURE), "--nucleus"], capture_output=True, text=True, timeout=300, env={"MMI_NO_GRAPH": "1"})
    assert p.returncode == 0 and "SELFTEST PASSED" in p.stdout, p.stdout + p.stderr
    assert "top_p = 1e-6 differs from the greedy stream in 0 of 72 tokens" in p.stdout, p.stdout
    assert "14 of 14 refusal checks held" in p.stdout, p.stdout
