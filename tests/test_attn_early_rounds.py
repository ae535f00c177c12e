"""k_lm_attn_wave's first rounds (requested before the offset is known) and its last round (odd and even round counts, one live row)
on the CPU kernel simulator: tests/attn_early_cases.py - ring depths around the rounds of one workgroup, unwrapped and wrapped, on
capacities that clamp the early loads, against the fp64 softmax of tests/attn_cases.py, and poison in the never-written slots."""
import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import attn_cases as ac
from tests import attn_early_cases as ec
from tests.lm_cases import cached_lm_state_dict


@pytest.fixture(scope="module")
def lm(sim_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=ac.ROWS, lib=sim_lib)


def test_case_list_covers_depths_wraps_and_capacities():
    ec.check_case_list()


@pytest.mark.parametrize("form,Dh,cap", ec.CASES)
def test_attention_equals_the_fp64_softmax(lm, form, Dh, cap):
    ec.check_fp64(lm, form, Dh, cap)


@pytest.mark.parametrize("pattern", ec.PATTERNS)
@pytest.mark.parametrize("form,Dh,cap", ec.CASES)
def test_poison_in_never_written_slots_changes_nothing(lm, form, Dh, cap, pattern):
    ec.check_unwritten(lm, form, Dh, cap, pattern)
