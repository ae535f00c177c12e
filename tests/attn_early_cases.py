"""Cases for the start and the end of k_lm_attn_wave's walk (one workgroup per pair, NS = 1: the path of the flagship step), shared by
tests/test_attn_early_rounds.py (simulator) and tests/test_c_attn_early_rounds_gpu.py (MI355X).  The kernel requests keys and values
before the session's offset is known - from slots clamped to cap - 1, not to L - 1 - zeroes the value rows of slots >= L afterwards
and walks the rounds in pairs, whatever their count.  The list is laid out for the first TWO rounds, so that it also holds a kernel
that requests both early and ends an odd count with a single round (scripts/experiments/attn_early_round1_single_tail.patch, measured
and not kept).  With R = 4 RPW NB, the rows one round of the workgroup covers (attn_cases.consts), every launch holds 16 rings of one
capacity (attn_cases' helpers carry 16 rows x 2 heads per launch):

  depths L in {1, R - 1, R, R + 1, 2R, 2R + 1, 3R, 3R + 1, 4R} that fit the capacity, unwrapped (offset L - 1): one round, odd and
  even round counts, a last round with one live row; the remaining rows are rings that have wrapped (L = cap), the newest row in
  slot 0, in slot cap - 1, mid-ring and elsewhere;
  capacities {5, R, 2R - 1, 2R, 4R + 5} - the early loads of rounds 0 and 1 clamp to cap - 1, reach exactly the end, or stay inside -
  and every depth of the list as a capacity, so that a wrapped ring exists at each depth.

Checks: the fp64 softmax under attn_cases' tolerance (GAMMA unchanged), and never-written slots (>= L) - keys and values - filled with
NaN, Inf, all-ones bytes and the largest finite values: the output is finite and equals the zero-filled run bit for bit."""
from __future__ import annotations

import dataclasses
from functools import lru_cache

import numpy as np

from tests import attn_cases as ac

PATHS = (ac.Path("wave", 1),)
SHAPES = (("bf16", 32), ("bf16", 128), ("fp8", 128), ("fp4", 128))
PATTERNS = ("nan", "garbage", "inf", "ff")


def round_rows(form: str, Dh: int) -> int:
    return ac.consts(form, Dh, 1)[2]


def depths(form: str, Dh: int):
    R = round_rows(form, Dh)
    return [1, R - 1, R, R + 1, 2 * R, 2 * R + 1, 3 * R, 3 * R + 1, 4 * R]


def capacities(form: str, Dh: int):
    R = round_rows(form, Dh)
    return sorted(set([5, R, 2 * R - 1, 2 * R, 4 * R + 5] + depths(form, Dh)))


def offsets_for(form: str, Dh: int, cap: int) -> np.ndarray:
    """16 offsets: every depth of the list that fits, unwrapped, then wrapped rings."""
    un = [L - 1 for L in depths(form, Dh) if L <= cap]
    wrapped = [cap, 2 * cap - 1, cap + cap // 2, 3 * cap, 4 * cap - 1, 2 * cap + 7 % cap, cap + 1 % cap, 5 * cap + cap // 3, cap + 2 * cap // 3,
               6 * cap + cap // 5, 7 * cap + 3 * cap // 4, 8 * cap + cap // 7, 9 * cap - 1, 10 * cap, 11 * cap + cap // 2]
    out = (un + wrapped)[:ac.ROWS]
    assert len(out) == ac.ROWS and len(un) >= 1 and len(un) < ac.ROWS
    return np.array(out, np.int64)


CASES = [(form, Dh, cap) for form, Dh in SHAPES for cap in capacities(form, Dh)]


@lru_cache(maxsize=2)
def launch(form: str, Dh: int, cap: int) -> ac.Launch:
    """attn_cases' random family on a ring of `cap` slots, at this file's offsets (mask and reference restated for them)."""
    lc = ac.build(form, Dh, "random", "B", cap=cap)
    offsets = offsets_for(form, Dh, cap)
    mask = ac.valid_mask(offsets, cap, lc.context)
    ref, A, p = ac.reference(lc.q, lc.Kd, lc.Vd, mask)
    return dataclasses.replace(lc, offsets=offsets, mask=mask, ref=ref, A=A, p=p)


def check_case_list():
    for form, Dh in SHAPES:
        R = round_rows(form, Dh)
        assert R == {("bf16", 32): 256, ("bf16", 128): 64, ("fp8", 128): 128, ("fp4", 128): 128}[(form, Dh)]
        caps = capacities(form, Dh)
        assert {5, R, 2 * R - 1, 2 * R}.issubset(caps) and max(caps) > 4 * R and set(depths(form, Dh)).issubset(caps)
        seen_un, seen_wrapped = set(), set()
        for cap in caps:
            offs = offsets_for(form, Dh, cap)
            seen_un |= {int(o) + 1 for o in offs if o + 1 <= cap}
            if (offs >= cap).any():
                seen_wrapped.add(cap)
        assert set(depths(form, Dh)) <= seen_un and set(depths(form, Dh)) <= seen_wrapped


def check_fp64(lm, form, Dh, cap):
    ac.check_tolerance(lm, launch(form, Dh, cap), PATHS, label=f"early/cap={cap}")


def _fill(ring: ac.Ring, rows_mask: np.ndarray, pattern: str) -> ac.Ring:
    """fill_rows' patterns, and two more: "inf" (bf16 +-Inf; e4m3 has none: its NaN with the sign set; 4-bit: code 6 under scale byte
    254 = 6 * 2^127, Inf once widened to fp32) and "ff" (every byte, scale bytes included, 0xFF: NaN in all three forms)."""
    if pattern in ("zero", "nan", "garbage"):
        return ac.fill_rows(ring, rows_mask, pattern)
    out = ring.copy()
    m = np.broadcast_to(rows_mask[:, None, :], out.codes.shape[:3])
    n = out.codes.shape[-1]
    if pattern == "ff":
        row, sc = np.full(n, 0xff, np.uint8), 0xff
    elif ring.form == "bf16":
        row, sc = np.tile(np.array([0x80, 0x7f, 0x80, 0xff], np.uint8), n // 4), 0          # +Inf, -Inf
    elif ring.form == "fp8":
        row, sc = np.full(n, 0xff, np.uint8), 0
    else:
        row, sc = np.full(n, 0xe6, np.uint8), 254
    out.codes[m] = row
    if out.scales is not None:
        out.scales[m] = sc
    return out


def check_unwritten(lm, form, Dh, cap, pattern):
    lc = launch(form, Dh, cap)
    if pattern in ("nan", "garbage"):
        ac.check_outside(lm, lc, pattern, PATHS)
        return
    never = ~ac.written_mask(lc.offsets, lc.cap)
    zero = ac.run(lm, lc, PATHS[0], _fill(lc.K, never, "zero"), _fill(lc.V, never, "zero"))
    V = _fill(lc.V, never, pattern)
    if never.any():
        with np.errstate(over="ignore", invalid="ignore"):
            assert not np.isfinite(V.decode()[np.broadcast_to(never[:, None, :], (ac.ROWS, ac.H, lc.cap))]).any()
    got = ac.run(lm, lc, PATHS[0], _fill(lc.K, never, pattern), V)
    assert np.isfinite(ac.bf16_bits_to_f32(got)).all(), f"{pattern} in never-written slots, {form} Dh={Dh} cap={cap}: output not finite"
    assert np.array_equal(got, zero), (f"{pattern} in never-written slots, {form} Dh={Dh} cap={cap}: differs from the zero-filled run, first at row "
                                       f"{np.argwhere(got != zero)[0][0]} (offsets {lc.offsets.tolist()})")
