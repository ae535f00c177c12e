"""Forking a live session into other slots on the CPU kernel simulator: tests/fork_cases.py through the same
kernel and engine sources the GPU runs."""
import re
from pathlib import Path

import pytest

from tests import fork_cases as fc

ROOT = Path(__file__).resolve().parent.parent


# ---- 1. + 2. continuation, bit for bit; neighbours untouched ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", fc.DEPTHS)
@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp4"])
def test_copy_continues_like_its_source_and_like_the_control(sim_lib, kv, d):
    fc.check_continuation("cpu", sim_lib, kv, d)


@pytest.mark.parametrize("d", fc.DEPTHS)
def test_seeded_draw_stream_continues_in_the_copy(sim_lib, d):
    fc.check_continuation("cpu", sim_lib, "bf16", d, seeded=True)


# ---- 3. several destinations ---------------------------------------------------------------------------------------------------------------
def test_three_destinations_in_one_call_then_three_seeds(sim_lib):
    fc.check_several_destinations("cpu", sim_lib)


# ---- 4. guided streams -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [False, True])
def test_guided_stream_copies_both_model_rows_and_the_condition(sim_lib, cross):
    fc.check_guided("cpu", sim_lib, cross)


@pytest.mark.parametrize("d", [1, 5])
def test_guided_stream_restored_from_a_snapshot_then_forked(sim_lib, d):
    fc.check_guided_after_restore("cpu", sim_lib, d)


# ---- 5. TTS machine, adapters ------------------------------------------------------------------------------------------------------------------
def test_copy_finishes_the_source_script(sim_lib):
    fc.check_tts_machine("cpu", sim_lib)


def test_copy_runs_on_the_source_adapter_slot(sim_lib):
    fc.check_adapter("cpu", sim_lib)


# ---- 6. many rows --------------------------------------------------------------------------------------------------------------------------------
def test_fork_across_the_32_and_64_row_tile_boundaries(sim_lib):
    fc.check_many_rows("cpu", sim_lib)


# ---- 7. log-probabilities ----------------------------------------------------------------------------------------------------------------------
def test_destination_logprob_rows_are_cleared(sim_lib):
    fc.check_logprobs("cpu", sim_lib)


# ---- 8. the codec -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 1, 3, 5])
def test_codec_copy_continues_like_its_source(sim_lib, f):
    fc.check_codec("cpu", sim_lib, f)


# ---- 9. the batcher -----------------------------------------------------------------------------------------------------------------------------
def test_batcher_fork(sim_lib):
    fc.check_batcher("cpu", sim_lib)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(sim_lib):
    fc.check_refusals("cpu", sim_lib)


# ---- 11. ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_prototypes_equal_the_ctypes_signatures():
    import ctypes as C
    from moshi_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "moshi_mi.h").read_text(), flags=re.S)
    assert re.search(r"int mmi_lm_fork_session\(mmi_lm\* lm, int32_t src, const int32_t\* dst, int32_t n_dst, mmi_stream stream\);", text)
    assert re.search(r"int mmi_mimi_fork_session\(mmi_mimi\* m, int32_t src, const int32_t\* dst, int32_t n_dst, mmi_stream stream\);", text)
    assert re.search(r"int mmi_batcher_fork\(mmi_batcher\* b, int64_t parent_channel, const mmi_row_sampling\* settings_or_null, "
                     r"int64_t\* channel_id\);", text)
    P, I = C.c_void_p, C.POINTER(C.c_int32)
    assert _capi.SIGNATURES["mmi_lm_fork_session"] == (C.c_int, [P, C.c_int32, I, C.c_int32, P])
    assert _capi.SIGNATURES["mmi_mimi_fork_session"] == (C.c_int, [P, C.c_int32, I, C.c_int32, P])
    assert _capi.SIGNATURES["mmi_batcher_fork"] == (C.c_int, [P, C.c_int64, C.POINTER(_capi.RowSampling), C.POINTER(C.c_int64)])
