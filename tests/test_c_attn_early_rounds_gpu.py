"""k_lm_attn_wave's first rounds (requested before the offset is known) and its last round (odd and even round counts, one live row)
on the MI355X: the case list of tests/attn_early_cases.py, as tests/test_attn_early_rounds.py runs it on the simulator, with what the
simulator never runs - the non-temporal ring loads, v_dot2, the DPP sums and the hardware widening."""
import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import attn_cases as ac
from tests import attn_early_cases as ec
from tests.lm_cases import cached_lm_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm(gpu_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=ac.ROWS, lib=gpu_lib)


@pytest.mark.parametrize("form,Dh,cap", ec.CASES)
def test_attention_equals_the_fp64_softmax(lm, form, Dh, cap):
    ec.check_fp64(lm, form, Dh, cap)


@pytest.mark.parametrize("pattern", ec.PATTERNS)
@pytest.mark.parametrize("form,Dh,cap", ec.CASES)
def test_poison_in_never_written_slots_changes_nothing(lm, form, Dh, cap, pattern):
    ec.check_unwritten(lm, form, Dh, cap, pattern)
