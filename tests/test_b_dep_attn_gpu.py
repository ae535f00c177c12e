"""The depth transformer's attention and the cross attention alone (`mmi_lm_debug_dep_attn`, `mmi_lm_debug_dep_attn_out_proj`,
`mmi_lm_debug_cross_attn`) on the MI355X: tests/dep_attn_cases.py - an fp64 softmax on crafted operands - against
k_dep_attn8<4>, k_dep_attn<16>, k_dep_attn<32>, k_dep_attn_out_proj and k_lm_cross_attn, with what the simulator never runs: the
hardware's expf and division, ds_bpermute butterflies, the LDS hand-over to the MFMA operand.  The whole list; the file's run time
is in profiles/dep_attn/README.md."""
from dataclasses import replace

import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import dep_attn_cases as dc
from tests.lm_cases import cached_lm_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm(gpu_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=16, lib=gpu_lib)


def one_session(lib, heads):
    cfg = replace(tiny_lm_config(), depformer_num_heads=heads)
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=1, lib=lib)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: s.id)
def test_depth_attention_equals_the_fp64_softmax(lm, shape):
    dc.check_dep_shape(lm, shape)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: s.id)
def test_depth_cache_rows_the_step_must_not_read_change_nothing(lm, shape):
    dc.check_dep_decoys(lm, shape)


def test_depth_attention_at_the_scoring_pass_rows(lm):
    dc.check_dep_score_rows(lm)


@pytest.mark.parametrize("heads", [2, 4])
def test_attention_inside_out_proj_equals_the_two_launches(gpu_lib, heads):
    """heads = 2: heads of 32, one per wave; 4: heads of 16, two per wave - the second pair of HPW = 2 is live."""
    dc.check_fused(one_session(gpu_lib, heads))


@pytest.mark.parametrize("family", dc.X_FAMILIES)
@pytest.mark.parametrize("Dh", dc.X_HEAD_DIMS)
def test_cross_attention_equals_the_fp64_softmax(lm, Dh, family):
    dc.check_cross(lm, Dh, family)


@pytest.mark.parametrize("Dh", dc.X_HEAD_DIMS)
def test_cross_positions_past_the_length_change_nothing(lm, Dh):
    dc.check_cross_outside(lm, Dh)


def test_refusals(lm, gpu_lib):
    cfg = replace(tiny_lm_config(), dep_q=12)
    twelve = LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cuda", max_batch=1, lib=gpu_lib)
    dc.check_refusals(lm, one_session(gpu_lib, 2), twelve)
