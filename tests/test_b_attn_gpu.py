"""The temporal decode attention alone (`mmi_lm_debug_attn`) on the MI355X: tests/attn_cases.py - an fp64 softmax on
crafted rings - against k_lm_attn_wave, k_lm_attn_split, k_lm_attn_combine and the merge by the last-arriving workgroup, with what
the simulator never runs: v_dot2_f32_bf16, the DPP group sums, v_cvt_pk_f32_fp8, v_cvt_scalef32_pk_f32_fp4, v_pk_fma_f32 and the
agent-scope arrival counter.  The whole grid; the file's run time is in profiles/attn_exact/README.md."""
import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import attn_cases as ac
from tests.lm_cases import cached_lm_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm(gpu_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=ac.ROWS, lib=gpu_lib)


@pytest.mark.parametrize("form,Dh,family,which", ac.GRID)
def test_attention_equals_the_fp64_softmax(lm, form, Dh, family, which):
    ac.check_family(lm, form, Dh, family, which)


@pytest.mark.parametrize("form,Dh,family,which", ac.OUTSIDE)
def test_largest_finite_values_outside_the_attended_part_change_nothing(lm, form, Dh, family, which):
    ac.check_outside(lm, ac.cached_build(form, Dh, family, which), "garbage")


@pytest.mark.parametrize("form,Dh,family,which", ac.OUTSIDE)
def test_nan_in_never_written_slots_changes_nothing(lm, form, Dh, family, which):
    ac.check_outside(lm, ac.cached_build(form, Dh, family, which), "nan")


def test_refusals(lm):
    ac.check_refusals(lm)
