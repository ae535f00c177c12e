"""struct mmi_lm_cfg_ext (mmi_lm_create_ext): the header's layout as gcc lays it out == the ctypes Structure of the binding, and
mmi_lm_cfg keeps its ABI-version-3 size."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_lm_cfg_ext_layout_equals_the_binding(tmp_path):
    import ctypes
    from moshi_amd import _capi
    fields = [n for n, *_ in _capi.LMCfgExt._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "moshi_mi.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(mmi_lm_cfg_ext));', '  printf("cfg %zu\\n", sizeof(mmi_lm_cfg));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mmi_lm_cfg_ext, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / "ext.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "ext"
    subprocess.check_call(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["."]) == ctypes.sizeof(_capi.LMCfgExt)
    assert int(got["cfg"]) == ctypes.sizeof(_capi.LMCfg)
    for f in fields:
        assert int(got[f]) == getattr(_capi.LMCfgExt, f).offset, f
    assert "mmi_lm_create_ext" in _capi.SIGNATURES
