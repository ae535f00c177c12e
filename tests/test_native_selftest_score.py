"""scripts/native_selftest.cpp --score, built against the CPU simulator like tests/test_native_selftest.py builds the other modes:
teacher-forced scoring through the C ABI alone - the recorded forced frames go through mmi_lm_score with commit = 1, its logits are held
to the recorded step logits, logp and argmax to the double-precision values from the returned logits, the following steps to the
oracle's record, and the entry points' refusal codes hold."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HIPSIM = ROOT / "tests" / "hipsim"
FIXTURE = ROOT / "tests" / "golden" / "native_selftest"


def test_native_selftest_score_mode_passes_on_the_simulator_build(sim_lib, tmp_path):
    sys.path.insert(0, str(HIPSIM))
    import build_sim
    exe = tmp_path / "native_selftest_sim"
    lib = Path(sim_lib.path)
    subprocess.check_call([build_sim._cxx(), "-O1", "-w", "-std=c++17", "-ffp-contract=off", "-pthread", "-DMMI_SELFTEST_SIM", f"-I{HIPSIM}",
                           f"-I{ROOT / 'include'}", str(ROOT / "scripts" / "native_selftest.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}",
                           "-o", str(exe)])
    p = subprocess.run([str(exe), str(FIXTURE), "--score"], capture_output=True, text=True, timeout=600, env={"MMI_NO_GRAPH": "1"})
    assert p.returncode == 0 and "SELFTEST PASSED" in p.stdout, p.stdout + p.stderr
    assert p.stdout.count("2 frames scored") == 2 and p.stdout.count("argmax differs in 0 sites") == 2, p.stdout
    assert p.stdout.count("0 of 54 token-ring outputs of the next steps differ") == 2, p.stdout
    assert "4 rows per pass" in p.stdout and "2 rows per pass" in p.stdout, p.stdout
    assert "9 of 9 refusal checks held" in p.stdout, p.stdout
