"""The depth transformer's attention and the cross attention alone (`mmi_lm_debug_dep_attn`, `mmi_lm_debug_dep_attn_out_proj`,
`mmi_lm_debug_cross_attn`) on the CPU kernel simulator: tests/dep_attn_cases.py - an fp64 softmax on crafted operands -
against the same kernel code the GPU runs, the whole list of the MI355X suite (tests/test_b_dep_attn_gpu.py).  What the simulator
cannot see - the hardware's expf and division, the LDS hand-over to the MFMA operand under real wave scheduling - is the GPU file's
part."""
from dataclasses import replace

import numpy as np
import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import attn_cases as ac
from tests import dep_attn_cases as dc
from tests.lm_cases import cached_lm_state_dict


@pytest.fixture(scope="module")
def lm(sim_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=16, lib=sim_lib)


def one_session(lib, device, heads):
    cfg = replace(tiny_lm_config(), depformer_num_heads=heads)
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device=device, max_batch=1, lib=lib)


# ---- the case list itself (numpy only) ------------------------------------------------------------------------------------------------------
def test_gamma_is_the_twins_measurement():
    """GAMMA re-measured the way DESIGN.md 8.19 measured it equals the figure recorded in dep_attn_cases; it is this list's own
    because it lies above the decode list's."""
    worst, where = dc.measure_gamma(verbose=False)
    assert abs(4 * worst - dc.GAMMA_MEASURED) < 0.1, (worst, where)
    assert dc.GAMMA_MEASURED > ac.GAMMA and where == "cross Dh=128 ramp_up"


def test_shapes_reach_every_branch_of_the_dispatch():
    runs = {(s.kernel, s.runs) for s in dc.SHAPES}
    assert runs == {("attn8", "attn8"), ("auto", "attn8"), ("auto", "rows16"), ("auto", "rows32"), ("rows16", "rows16"), ("rows32", "rows32")}
    auto16 = {(s.Dh, s.steps) for s in dc.SHAPES if (s.kernel, s.runs) == ("auto", "rows16")}
    assert {(32, 9), (64, 16), (4, 8), (20, 8)} <= auto16          # 9..16 positions, and a head dim that is no multiple of 8
    for s in dc.SHAPES:
        seen = {dc.rows_of(s, k, f) for k in s.ks for f in dc.FAMILIES}
        assert seen == set(dc.ROWS), s.id
        assert all((r * dc.H) % 4 for r in dc.ROWS)


def test_needles_sit_where_their_names_say():
    for s in (dc.SHAPES[0], next(x for x in dc.SHAPES if x.Dh == 20), next(x for x in dc.SHAPES if x.steps == 20)):
        for k in s.ks:
            for fam, pos in (("needle:pos0", 0), ("needle:k-1", max(k - 1, 0)), ("needle:k", k), ("needle:tail", k // 2)):
                lc = dc.build_dep(s, k, fam)
                assert (lc.hot == pos).all() and pos <= k
                dc.check_needle_ref(lc.p, lc.V, lc.hot, lc.mask)
            lc = dc.build_dep(s, k, "needle:tail")
            n = 8 if s.Dh % 8 == 0 else 1
            assert (lc.K[:, :, :, :s.Dh - n] == lc.K[:, :, :1, :s.Dh - n]).all()      # the rivals differ in the last chunk / lane only
    for Dh in dc.X_HEAD_DIMS:
        rp, cap = dc.x_consts(Dh)
        L = set(dc.x_lengths(Dh).tolist())
        assert {1, 2, rp - 1, rp, rp + 1, 2 * rp - 1, 2 * rp, 2 * rp + 1, 3 * rp + 1, cap - 1, cap} <= L and cap == 5 * rp + 3
        lc = dc.build_cross(Dh, "two_needles")
        two = [(b, h) for b in range(dc.XROWS) for h in range(dc.XH) if lc.hot[b, h, 0] % rp != lc.hot[b, h, 1] % rp]
        assert len(two) >= dc.XROWS                                 # two needles in different slots on most pairs


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: s.id)
def test_depth_attention_equals_the_fp64_softmax(lm, shape):
    dc.check_dep_shape(lm, shape)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: s.id)
def test_depth_cache_rows_the_step_must_not_read_change_nothing(lm, shape):
    dc.check_dep_decoys(lm, shape)


def test_depth_attention_at_the_scoring_pass_rows(lm):
    dc.check_dep_score_rows(lm)


@pytest.mark.parametrize("heads", [2, 4])
def test_attention_inside_out_proj_equals_the_two_launches(sim_lib, heads):
    """heads = 2: heads of 32, one per wave; 4: heads of 16, two per wave - the second pair of HPW = 2 is live."""
    dc.check_fused(one_session(sim_lib, "cpu", heads))


@pytest.mark.parametrize("family", dc.X_FAMILIES)
@pytest.mark.parametrize("Dh", dc.X_HEAD_DIMS)
def test_cross_attention_equals_the_fp64_softmax(lm, Dh, family):
    dc.check_cross(lm, Dh, family)


@pytest.mark.parametrize("Dh", dc.X_HEAD_DIMS)
def test_cross_positions_past_the_length_change_nothing(lm, Dh):
    dc.check_cross_outside(lm, Dh)


def test_refusals(lm, sim_lib):
    cfg = replace(tiny_lm_config(), dep_q=12)
    twelve = LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=1, lib=sim_lib)
    dc.check_refusals(lm, one_session(sim_lib, "cpu", 2), twelve)
