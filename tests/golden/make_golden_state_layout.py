"""Writes tests/golden/lm_state_layout.json: the layout and the start-up bytes of the LM engine's streaming state per configuration
of tests/state_layout_cases.py (what is recorded and why: that file's docstring).

    python tests/golden/make_golden_state_layout.py                 # the simulator's values (CPU)
    MMI_LIB_PATH=<parent's libmoshi_mi.so> python tests/golden/make_golden_state_layout.py --device-launch-lists   # on an MI355X

The file was recorded on the commit BEFORE the streaming-state table (the parent of the commit that added this script), against
that commit's simulator library: the table must reproduce the hand-written lists it replaced, byte for byte.  Re-running the script
on a later tree must reproduce the file with no diff; a diff is a change of the snapshot format.

`--device-launch-lists` adds `device_launch_sha256` to the configurations whose launch list on the device differs from the
simulator's (the simulator has no graph capture, and a launch chosen by the device's CU count may differ).  It keeps every other
value of the file as it is, and it was run with MMI_LIB_PATH naming the PARENT commit's product library: a device value is never
recorded from the tree under test."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def main():
    from tests import state_layout_cases as sl
    if "--device-launch-lists" in sys.argv:
        assert os.environ.get("MMI_LIB_PATH"), "name the parent commit's library with MMI_LIB_PATH"
        out = sl.load_golden()
        for name in sl.CONFIGS:
            m = sl.measure(name, "cuda", None, steps=False)
            for k in ("state_bytes", "regions", "start_sha256"):          # what the GPU test asserts from the simulator's record
                if m[k] != out[name][k] and not (k == "start_sha256" and name in sl.GEMM_AT_START):
                    print(name, k, "differs on the device from the simulator's record", flush=True)
            got = m["launch_sha256"]
            out[name].pop("device_launch_sha256", None)
            if got != out[name]["launch_sha256"]:
                out[name]["device_launch_sha256"] = got
            print(name, "device launch list:", "as the simulator's" if got == out[name]["launch_sha256"] else got, flush=True)
    else:
        os.environ["MMI_NO_GRAPH"] = "1"        # the simulator has no graph capture (tests/conftest.py sim_lib)
        sys.path.insert(0, str(ROOT / "tests" / "hipsim"))
        import build_sim
        from moshi_amd import _capi
        lib = _capi.load(os.environ.get("MMI_SIM_LIB") or build_sim.build())
        old = sl.load_golden() if sl.GOLDEN.exists() else {}
        out = {}
        for name in sl.CONFIGS:
            out[name] = sl.measure(name, "cpu", lib)
            del out[name]["launch_text"]                             # (the file keeps its hash)
            if "device_launch_sha256" in old.get(name, {}):         # recorded on the device from the parent's library: kept
                out[name]["device_launch_sha256"] = old[name]["device_launch_sha256"]
            print(name, out[name]["state_bytes"], out[name]["start_sha256"][:12], out[name]["step_sha256"][:12], flush=True)
    sl.GOLDEN.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print("wrote", sl.GOLDEN)


if __name__ == "__main__":
    main()
