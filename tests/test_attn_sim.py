"""The temporal decode attention alone (`mmi_lm_debug_attn`) on the CPU kernel simulator: tests/attn_cases.py - an fp64
softmax on crafted rings - against the same kernel code the GPU runs.  The simulator walks a launch of 16 rings in well under a
second, so it runs the whole grid of the MI355X suite (tests/test_b_attn_gpu.py): both kernels, the three ring forms, head dims
32 / 64 / 128, and per case the five paths of attn_cases.PATHS.  What it cannot see - v_dot2, the DPP sums, the hardware widening, the
agent-scope counter - is the GPU file's part."""
import numpy as np
import pytest

from moshi_amd import LMModel
from moshi_amd.config import tiny_lm_config
from tests import attn_cases as ac
from tests.lm_cases import cached_lm_state_dict


@pytest.fixture(scope="module")
def lm(sim_lib):
    cfg = tiny_lm_config()
    return LMModel(cached_lm_state_dict(cfg, 21), cfg, device="cpu", max_batch=ac.ROWS, lib=sim_lib)


# ---- the reference itself ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,context", [(7, 7), (7, 3), (5, 1), (8, 5)])
def test_mask_rule_equals_a_ring_written_step_by_step(cap, context):
    """valid_mask against the plainest statement: write position t into slot t % cap for t = 0 .. off, attend what is still there and
    inside the window."""
    offsets = np.arange(0, 4 * cap + 2, dtype=np.int64)
    got = ac.valid_mask(offsets, cap, context)
    for off in offsets:
        held = np.full(cap, -1, np.int64)
        for t in range(int(off) + 1):
            held[t % cap] = t
        assert np.array_equal(got[off], (held >= 0) & (off - held < context)), (cap, context, off)
        assert np.array_equal(ac.written_mask(offsets, cap)[off], held >= 0)


def test_ring_decoders_are_exact():
    """e4m3 by its rule against torch's conversion on all 254 numbers; bf16 and the 4-bit form round-trip what `encode` wrote."""
    import torch
    b = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(b).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(ac.E4M3[np.isfinite(want)], want[np.isfinite(want)]) and np.isnan(ac.E4M3[[0x7f, 0xff]]).all()
    x = np.random.default_rng(3).standard_normal((1, 1, 9, 32), dtype=np.float32)
    for form in ac.FORMS:
        d = ac.encode(form, x).decode()
        assert np.array_equal(ac.encode(form, d).decode(), d) and np.array_equal(ac.bf16_round(d), d)
    assert np.array_equal(ac.encode("bf16", x).decode(), ac.bf16_round(x))


@pytest.mark.parametrize("form", ac.FORMS)
def test_fp32_twin_stays_inside_the_tolerance(form):
    """GAMMA is 4 x the twin's worst ratio over the whole list (attn_cases.measure_gamma, 20 s): here the families that set it."""
    for Dh, family in ((128, "ramp_up"), (32, "peaky")):
        lc = ac.build(form, Dh, family, "B")
        tw = ac.fp32_twin(lc.q, lc.Kd, lc.Vd, lc.mask).astype(np.float64)
        assert (np.abs(tw - lc.ref) <= 0.5 * ac.tolerance(lc.ref, lc.A)).all()


def test_lengths_cover_what_the_kernels_distinguish():
    for form in ac.FORMS:
        for Dh in ac.HEAD_DIMS:
            rpw, nb, g1 = ac.consts(form, Dh, 1)
            cap = ac.capacity(form, Dh)
            assert cap % rpw and cap >= 517
            A, B = ac.offset_sets(form, Dh)
            Ls = set(np.minimum(np.concatenate([A, B]) + 1, cap).tolist())
            for G in (g1, 3 * g1):
                assert {1, 2, rpw - 1, rpw, rpw + 1, G - 1, G, G + 1, 2 * G + 1, 3 * G - 1, 255, 256, 257, 513, cap - 1, cap} <= Ls
            ends = set((B[B >= cap] % cap).tolist())
            assert {0, cap - 1, cap // 2} <= ends
            solo = ac.solo_rows(form, Dh)                 # one launch holds pairs walked alone and pairs merged by the last arriver
            for offs in (A, B):
                L = np.minimum(offs + 1, cap)
                assert (L <= solo).any() or offs is B
                assert (L > solo).any()


def test_every_ring_carries_a_needle_on_every_named_position():
    """What the grid runs, read from the launches' own `note["hot"]`: on every ring of set B - unwrapped and wrapped, the newest row in
    slot 0, in slot cap - 1 and mid-ring - a bit-for-bit needle sits on slot 0, on L - 1, on the newest and on the oldest row and on
    every group, round and chunk edge; set A's rings carry slot 0, L - 1, newest and oldest; the windowed needle sits on the oldest
    position of the window and on the newest row.  (check_needle_placement restates each slot from the offset in every needle test.)"""
    grid = {(f, w) for _, _, f, w in ac.GRID}
    assert {(f"needle:{k}", "B") for k in range(7)} | {("needle:0", "A"), ("needle:1", "A"), ("needle:shares", "A"), ("needle:shares", "B"),
                                                         ("wneedle", "A"), ("wneedle", "B")} <= grid
    form, Dh = "fp8", 64
    cap = ac.capacity(form, Dh)
    for which, kinds in (("B", range(7)), ("A", range(2))):
        seen = [dict() for _ in range(ac.ROWS)]
        for k in kinds:
            lc = ac.build(form, Dh, f"needle:{k}", which)
            ac.check_needle_placement(lc)
            for b in range(ac.ROWS):
                for h in range(ac.H):
                    seen[b][lc.note["names"][b][h]] = int(lc.note["hot"][b, h, 0])
        offs = ac.offset_sets(form, Dh)[0 if which == "A" else 1]
        assert sum(o >= cap for o in offs) >= 2
        for b, off in enumerate(int(o) for o in offs):
            L = min(off + 1, cap)
            assert set(seen[b]) == set(ac.NAMED if which == "B" else ac.NAMED[:4])
            assert (seen[b]["slot0"], seen[b]["last"], seen[b]["newest"]) == (0, L - 1, off % cap)
            assert seen[b]["oldest"] == ((off + 1) % cap if off + 1 >= cap else 0)
    B = ac.offset_sets(form, Dh)[1]
    ends = {int(o) % cap for o in B if o >= cap}
    assert {0, cap - 1, cap // 2} <= ends                  # so "newest" was slot 0, cap - 1 and mid-ring, "oldest" slot 1, 0 and mid-ring + 1


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
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
