"""Cases for the depth transformer's attention and the cross attention ALONE (`mmi_lm_debug_dep_attn`, `mmi_lm_debug_dep_attn_out_proj`,
`mmi_lm_debug_cross_attn`), shared by the simulator suite (tests/test_dep_attn_sim.py) and the MI355X suite
(tests/test_b_dep_attn_gpu.py): k_dep_attn8<4>, k_dep_attn<16>, k_dep_attn<32>, k_dep_attn_out_proj and k_lm_cross_attn on operands built
so that each of their paths matters, against a softmax in fp64.

The reference is `attn_cases.reference` unchanged, on the bf16 operands widened exactly; the mask is j <= k for the depth attention
(micro-step k of a frame attends positions 0 .. k: rows < k of the frame's cache and the newest row, which is in `qkv`) and t < len[b]
for the cross attention.  The tolerance is `attn_cases.tolerance`, the rule unchanged, with a GAMMA of this list's own (`tolerance`
below): `measure_gamma` runs `attn_cases.fp32_twin` over every tolerance launch below - in chunks of 5 positions for the depth cases
(the twin then rescales inside 32 positions, in an order no kernel uses), 37 for the cross cases - and 4 x its worst ratio
|twin - ref| / (2^-24 A_d) is GAMMA_MEASURED.  The worst ratio is 90.29 (cross attention, head dim 128, the rising ramp, row 9 of 22
positions; the depth list's worst is 74.91: 20 steps, k = 16, head dim 32, the rising ramp), above the 50.08 of the decode list, so
attn_cases.GAMMA = 200.3 does NOT cover this list and is left alone: the ramps here put scores of about 100 - whose fp32 spacing is
2^-17 = 128 x 2^-24 - on NEIGHBOURING positions of rows that are 2 .. 83 positions long, where the two largest weights are of the same
order; the decode list's ramps run over hundreds of slots (profiles/dep_attn/README.md)."""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np
import torch

from tests import attn_cases as ac
from tests.kv4_cases import bf16_bits_to_f32

GAMMA_MEASURED = 361.2            # 4 x 90.29 (measure_gamma; test_dep_attn_sim re-measures it).  Above attn_cases.GAMMA: this list's own
H = 3                             # depth launches: B * H is no multiple of the 4 waves of k_dep_attn8<4>
ROWS = (1, 5, 18)                 # one and two 16-row tiles of the packed output, and a single pair
SCORE_ROWS = 128                  # the scoring pass's rows: four 32-row tiles
BF16_MAX = 0x7f7f                 # the largest finite bf16
BF16_NAN = 0x7fc0


# ---- depth attention: the shapes -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    kernel: str                   # what the test asks the tap for: "auto" / "attn8" / "rows16" / "rows32"
    runs: str                     # the kernel that must run
    Dh: int
    steps: int
    ks: tuple

    @property
    def id(self):
        return f"{self.kernel}-{self.runs}-Dh{self.Dh}-steps{self.steps}"


def _uniq(xs):
    out = []
    for x in xs:
        if x not in out and x <= xs[-1]:               # (steps = 17 has no micro-step 17)
            out.append(x)
    return tuple(out)


def step_choice(Dh: int, steps: int) -> str:
    """The step's dispatch, restated: k_dep_attn8 for a head dim that is a multiple of 8 and at most 8 positions; else the general
    kernel with 16 rows in registers, 32 above 16 positions."""
    if Dh % 8 == 0 and steps <= 8:
        return "attn8"
    return "rows32" if steps > 16 else "rows16"


SHAPES = tuple(
    [Shape("attn8", "attn8", Dh, 8, tuple(range(8))) for Dh in (8, 24, 32, 64)] + [Shape("attn8", "attn8", 32, 3, (0, 1, 2))]
    + [Shape("auto", "attn8", 32, 8, tuple(range(8)))]
    + [Shape("auto", "rows16", Dh, steps, _uniq((0, 1, 7, 8, steps - 1))) for Dh in (32, 64) for steps in (9, 16)]
    + [Shape("auto", "rows16", Dh, 8, (0, 1, 7)) for Dh in (4, 20)]
    + [Shape("auto", "rows32", Dh, steps, _uniq((0, 1, 15, 16, 17, steps - 1))) for Dh in (32, 64) for steps in (17, 20, 32)]
    + [Shape("rows16", "rows16", 32, 8, tuple(range(8))), Shape("rows32", "rows32", 32, 8, tuple(range(8)))])
assert all(max(s.ks) < s.steps for s in SHAPES) and all(s.kernel != "auto" or step_choice(s.Dh, s.steps) == s.runs for s in SHAPES)

TOLERANCE_FAMILIES = ("random", "flat", "peaky", "ramp_up", "ramp_down")
NEEDLE_FAMILIES = ("needle:pos0", "needle:k-1", "needle:k", "needle:tail")
FAMILIES = TOLERANCE_FAMILIES + NEEDLE_FAMILIES


def rows_of(shape: Shape, k: int, family: str) -> int:
    """1, 5 or 18 rows, walking with the shape, the micro-step and the family so that every kernel sees all three."""
    return ROWS[(SHAPES.index(shape) + k + FAMILIES.index(family)) % 3]


def _needle_amp(Dh: int, n: int) -> float:
    """The power of two a with 2 a n / sqrt(Dh) >= 45: a key that differs from its rivals by 2 a q in n elements outscores them by 45,
    a weight of e^-45 each."""
    a = 1.0
    while 2 * a * n / np.sqrt(Dh) < 45:
        a *= 2
    return a


@dataclass
class Dep:
    """One launch: micro-step k of `rows` rows.  K / V hold every position 0 .. steps - 1 (bf16 values); the tap gets rows < k in the
    caches and row k in qkv."""
    shape: Shape
    k: int
    family: str
    rows: int
    heads: int
    q: np.ndarray                  # fp32 [rows, heads, Dh]
    K: np.ndarray                  # fp32 [rows, heads, steps, Dh]
    V: np.ndarray
    mask: np.ndarray               # bool [rows, steps]: j <= k
    ref: np.ndarray = None
    A: np.ndarray = None
    p: np.ndarray = None
    hot: np.ndarray = None         # int [rows, H]: the needle's position
    note: dict = field(default_factory=dict)


def build_dep(shape: Shape, k: int, family: str, rows: int = None, seed: int = 0, heads: int = H) -> Dep:
    Dh, steps, H = shape.Dh, shape.steps, heads
    rows = rows or rows_of(shape, k, family)
    rng = np.random.default_rng([seed, 11, Dh, steps, k, FAMILIES.index(family), rows])
    f = np.float32
    K = rng.standard_normal((rows, H, steps, Dh), dtype=f)
    V = rng.standard_normal((rows, H, steps, Dh), dtype=f)
    hot = None
    if family in ("random", "peaky"):
        q = rng.standard_normal((rows, H, Dh), dtype=f) * f(4.0 if family == "peaky" else 1.0)
    elif family == "flat":
        # all scores equal (and not zero): every position holds the same key per (row, head)
        q = rng.standard_normal((rows, H, Dh), dtype=f)
        K = np.repeat(K[:, :, :1], steps, axis=2)
    elif family in ("ramp_up", "ramp_down"):
        # key j = c_j sg + noise, scores c_j sqrt(Dh) from 2 to 102 over positions 0 .. steps - 1; ramp_down: the same keys under -q
        sg = ac._signs(rng, (rows, H, Dh))
        c = (2.0 + 100.0 * np.arange(steps, dtype=f) / max(steps - 1, 1)) / np.sqrt(f(Dh))
        K = c[None, None, :, None] * sg[:, :, None, :] + K * f(0.05)
        q = sg if family == "ramp_up" else -sg
    elif family.startswith("needle:"):
        # ONE key per (row, head) takes the whole weight: the output is its value row bit for bit
        kind = family.split(":")[1]
        q = ac._signs(rng, (rows, H, Dh))
        V = ac._needle_values(rng, rows * H * steps, Dh).reshape(rows, H, steps, Dh)      # every row distinct from the needle's with
        pos = {"pos0": 0, "k-1": max(k - 1, 0), "k": k, "tail": k // 2}[kind]            # overwhelming probability (asserted)
        hot = np.full((rows, H), pos, np.int64)
        if kind == "tail":
            # the rivals differ from the needle only in the last 16-byte chunk of the head (k_dep_attn8's lane c = Dh / 8 - 1), or,
            # where the head is no whole chunks, in its last lane (k_dep_attn's lane Dh - 1)
            n = 8 if Dh % 8 == 0 else 1
            a = f(_needle_amp(Dh, n))
            K = np.repeat((f(2.0) * q)[:, :, None, :], steps, axis=2)
            K[..., Dh - n:] = -a * q[:, :, None, Dh - n:]
            K[:, :, pos, Dh - n:] = a * q[..., Dh - n:]
        else:
            K[:, :, pos] = f(2 * _needle_amp(Dh, Dh)) * q                                # scores a sqrt(Dh) >= 45 against N(0, 1)
    else:
        raise KeyError(family)
    q, K, V = ac.bf16_round(q), ac.bf16_round(K), ac.bf16_round(V)
    mask = np.broadcast_to(np.arange(steps)[None, :] <= k, (rows, steps)).copy()
    ref, A, p = ac.reference(q, K, V, mask)
    return Dep(shape, k, family, rows, heads, q, K, V, mask, ref, A, p, hot)


def _bits(x: np.ndarray) -> np.ndarray:
    """bf16 values held in fp32 -> their bf16 bits (exact)."""
    x = np.ascontiguousarray(x, np.float32)
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def dep_operands(lc: Dep, later: str = "zero", at_k: str = "zero"):
    """(qkv, kc, vc) as uint16 bf16 bits.  Cache rows < k hold the frame's keys / values; row k (which the kernel overwrites and must
    never read) holds `at_k`, rows > k `later`: "zero", "max" (the largest finite bf16, signs alternating) or "nan"."""
    k, rows = lc.k, lc.rows
    Dh, steps = lc.shape.Dh, lc.shape.steps
    qkv = np.concatenate([_bits(lc.q).reshape(rows, -1), _bits(lc.K[:, :, k]).reshape(rows, -1), _bits(lc.V[:, :, k]).reshape(rows, -1)], 1)
    fill = {"zero": np.zeros(Dh, np.uint16), "nan": np.full(Dh, BF16_NAN, np.uint16),
            "max": np.where(np.arange(Dh) % 2 == 0, BF16_MAX, BF16_MAX | 0x8000).astype(np.uint16)}
    caches = []
    for X in (lc.K, lc.V):
        c = _bits(X).copy()
        c[:, :, k] = fill[at_k]
        c[:, :, k + 1:] = fill[later]
        caches.append(np.ascontiguousarray(c))
    return np.ascontiguousarray(qkv), caches[0], caches[1]


def _dev(lm, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(lm.device).view(torch.bfloat16)


def run_dep(lm, lc: Dep, kernel: str = None, later: str = "zero", at_k: str = "zero") -> np.ndarray:
    """The tap on a launch -> bf16 bits uint16 [rows, H, Dh], after the checks every launch gets: the kernel that ran is the one the
    shape names, cache rows != k are byte for byte what went in, row k is the k / v thirds of qkv."""
    qkv, kc, vc = dep_operands(lc, later, at_k)
    H = lc.heads
    tk, tv = _dev(lm, kc), _dev(lm, vc)
    out, ran = lm.debug_dep_attn(_dev(lm, qkv), tk, tv, H, lc.k, kernel=kernel or lc.shape.kernel)
    want = lc.shape.runs if kernel is None else (step_choice(lc.shape.Dh, lc.shape.steps) if kernel == "auto" else kernel)
    assert ran == want, f"{lc.shape.id} k={lc.k}: {ran} ran, the step would run {want}"
    HD = H * lc.shape.Dh
    for name, t, before, third in (("keys", tk, kc, 1), ("values", tv, vc, 2)):
        after = ac.bf16_bits(t)
        others = np.arange(lc.shape.steps) != lc.k
        assert np.array_equal(after[:, :, others], before[:, :, others]), f"{lc.shape.id} k={lc.k}: the {name} cache changed outside row k"
        assert np.array_equal(after[:, :, lc.k].reshape(lc.rows, HD), qkv[:, third * HD:(third + 1) * HD]), \
            f"{lc.shape.id} k={lc.k}: row k of the {name} cache is not the row of qkv"
    return ac.bf16_bits(out).reshape(lc.rows, H, lc.shape.Dh)


def tolerance(ref: np.ndarray, A: np.ndarray) -> np.ndarray:
    """attn_cases.tolerance with this list's GAMMA: 2^-8 |ref_d| + GAMMA_MEASURED 2^-24 A_d (+ FLOOR below the normal range)."""
    return ac.tolerance(ref, A) + (GAMMA_MEASURED - ac.GAMMA) * 2.0 ** -24 * A


STATS: dict = {}                  # label -> worst |out - ref| / tolerance seen in this process


def _within(got_bits: np.ndarray, ref: np.ndarray, A: np.ndarray, label: str, against: np.ndarray = None):
    """Worst |out - against| / tolerance(ref, A) (against = ref by default), printed before it is asserted."""
    got = bf16_bits_to_f32(got_bits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - (ref if against is None else against)) / tolerance(ref, A)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst = float(ratio.max())
    key = label.split(" ")[0]
    STATS[key] = max(STATS.get(key, 0.0), worst)
    print(f"{label}: worst |out - {'ref' if against is None else 'k_dep_attn8'}| / tolerance = {worst:.3f}")
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return f"{label}: {worst:.3g} x the tolerance at {tuple(int(x) for x in i)}: {got[i]!r} against {(ref if against is None else against)[i]!r}"
    return None


def check_needle_ref(p: np.ndarray, V: np.ndarray, hot: np.ndarray, live: np.ndarray):
    """The reference gives the needle a weight of at least 1 - 2^-30, and no other attended row holds its values."""
    bi, hi = np.meshgrid(np.arange(hot.shape[0]), np.arange(hot.shape[1]), indexing="ij")
    w = p[bi, hi, hot]
    assert (w >= 1 - 2.0 ** -30).all(), f"the reference gives a needle only {w.min()!r}"
    want = V[bi, hi, hot]
    same = (V == want[:, :, None, :]).all(-1) & live[:, None, :]
    assert (same.sum(-1) == 1).all(), "another attended row holds the needle's values"
    return want


def check_dep_shape(lm, shape: Shape):
    """Every family at every micro-step of one shape."""
    bad = []
    for k in shape.ks:
        for family in FAMILIES:
            lc = build_dep(shape, k, family)
            got = run_dep(lm, lc)
            label = f"{shape.id} k={k} {family} rows={lc.rows}"
            if family in TOLERANCE_FAMILIES:
                msg = _within(got, lc.ref, lc.A, label)
                if shape.kernel in ("rows16", "rows32") and shape.kernel != step_choice(shape.Dh, shape.steps):
                    # a forced general kernel where the step runs k_dep_attn8: also inside the tolerance of k_dep_attn8's output
                    other = bf16_bits_to_f32(run_dep(lm, lc, kernel="attn8")).astype(np.float64)
                    msg = msg or _within(got, lc.ref, lc.A, label + " vs attn8", against=other)
                if msg:
                    bad.append(msg)
            else:
                want = check_needle_ref(lc.p, lc.V, lc.hot, lc.mask)
                if not np.array_equal(got, _bits(want)):
                    b, h, _ = np.argwhere(got != _bits(want))[0]
                    bad.append(f"{label}: row {b} head {h}, needle on position {int(lc.hot[b, h])}: {bf16_bits_to_f32(got[b, h, :4])} "
                               f"against {want[b, h, :4]}")
    assert not bad, " | ".join(bad[:6]) + (f" | and {len(bad) - 6} more" if len(bad) > 6 else "")


def check_dep_decoys(lm, shape: Shape):
    """What the cache holds where micro-step k must not look changes nothing, bit for bit against the run with zeros there: rows k + 1
    .. steps - 1 hold the largest finite bf16, then NaN; row k itself holds NaN before the call."""
    for k in shape.ks:
        lc = build_dep(shape, k, "random")
        zero = run_dep(lm, lc)
        assert np.isfinite(bf16_bits_to_f32(zero)).all()
        for later, at_k in (("max", "zero"), ("nan", "zero"), ("zero", "nan"), ("nan", "nan")):
            got = run_dep(lm, lc, later=later, at_k=at_k)
            assert np.array_equal(got, zero), f"{shape.id} k={k}: {later} in rows > k, {at_k} in row k: differs from the run on zeros there"


def check_dep_score_rows(lm):
    """128 rows - the scoring pass's - in four 32-row tiles of the packed output."""
    shape = next(s for s in SHAPES if s.kernel == "auto" and s.runs == "attn8")
    for k, family in ((7, "random"), (3, "needle:k")):
        lc = build_dep(shape, k, family, rows=SCORE_ROWS)
        got = run_dep(lm, lc)
        if family == "random":
            msg = _within(got, lc.ref, lc.A, f"{shape.id} k={k} {family} rows={SCORE_ROWS}")
            assert not msg, msg
        else:
            assert np.array_equal(got, _bits(check_needle_ref(lc.p, lc.V, lc.hot, lc.mask)))
    shape = next(s for s in SHAPES if s.runs == "rows16" and s.Dh == 20)
    lc = build_dep(shape, 7, "random", rows=SCORE_ROWS)
    msg = _within(run_dep(lm, lc), lc.ref, lc.A, f"{shape.id} k=7 random rows={SCORE_ROWS}")
    assert not msg, msg


# ---- the attention inside out_proj ----------------------------------------------------------------------------------------------------------
def check_fused(lm):
    """On a one-session handle, for every micro-step 1 .. dep_q - 1 of both depth layers and every family: the fused launch and the two
    launches it replaces agree bit for bit in the output row and in both caches, and the attention part of the two-launch form - read
    through debug_dep_attn on the same operands - is inside the tolerance of the reference (a needle: its value row, bit for bit)."""
    cfg = lm.config
    Hd, Dh, steps = cfg.depformer_num_heads, cfg.depformer_dim // cfg.depformer_num_heads, cfg.dep_q
    shape = Shape("auto", step_choice(Dh, steps), Dh, steps, tuple(range(1, steps)))
    bad = []
    for layer in range(cfg.depformer_num_layers):
        for k in shape.ks:
            for family in FAMILIES:
                lc = build_dep(shape, k, family, rows=1, seed=1 + layer, heads=Hd)
                qkv, kc, vc = dep_operands(lc, later="nan", at_k="nan")
                x = ac.bf16_round(np.random.default_rng([5, layer, k]).standard_normal(cfg.depformer_dim, dtype=np.float32))
                res = {}
                for fused in (True, False):
                    tk, tv = _dev(lm, kc[0]), _dev(lm, vc[0])
                    out, att, ran = lm.debug_dep_attn_out_proj(layer, k, _dev(lm, qkv[0]), tk, tv, _dev(lm, _bits(x)), fused=fused)
                    assert ran == ("fused" if fused else "attn8"), ran
                    res[fused] = (ac.bf16_bits(out), ac.bf16_bits(tk), ac.bf16_bits(tv), None if att is None else ac.bf16_bits(att))
                label = f"fused H={Hd} layer {layer} k={k} {family}"
                for what, a, b in zip(("output row", "key cache", "value cache"), res[True][:3], res[False][:3]):
                    if not np.array_equal(a, b):
                        bad.append(f"{label}: the {what} differs between the fused launch and the two launches")
                alone = run_dep(lm, lc, later="nan", at_k="nan")
                if not np.array_equal(alone.reshape(-1), res[False][3]):
                    bad.append(f"{label}: the attention of the two-launch form is not what debug_dep_attn gives")
                if family in TOLERANCE_FAMILIES:
                    msg = _within(alone, lc.ref, lc.A, label)
                    if msg:
                        bad.append(msg)
                elif not np.array_equal(alone, _bits(check_needle_ref(lc.p, lc.V, lc.hot, lc.mask))):
                    bad.append(f"{label}: not the needle's value row")
    assert not bad, " | ".join(bad[:6]) + (f" | and {len(bad) - 6} more" if len(bad) > 6 else "")


# ---- cross attention --------------------------------------------------------------------------------------------------------------------------
XH, XROWS = 2, 16
X_HEAD_DIMS = (32, 64, 128)
X_TOLERANCE = ("random", "flat", "peaky", "ramp_up", "ramp_down", "two_needles", "underflow")
X_NEEDLES = ("needle:pos0", "needle:last", "needle:pass_first", "needle:pass_last", "needle:tail_first")
X_FAMILIES = X_TOLERANCE + X_NEEDLES


def x_consts(Dh: int):
    """(RP, cap): position slots per pass of k_lm_cross_attn (64 lanes / (Dh / 8) chunk lanes), and 5 RP + 3 positions."""
    rp = 512 // Dh
    return rp, 5 * rp + 3


def x_lengths(Dh: int) -> np.ndarray:
    rp, cap = x_consts(Dh)
    fixed = [1, 2, rp - 1, rp, rp + 1, 2 * rp - 1, 2 * rp, 2 * rp + 1, 3 * rp + 1, cap - 1, cap]
    more = np.random.default_rng([3, Dh]).integers(1, cap + 1, XROWS - len(fixed)).tolist()
    return np.array(fixed + more, np.int32)


def x_named(Dh: int, L: int) -> dict:
    """Where the needle goes by name on a row of L positions (clamped to L - 1): position 0, L - 1, the first and the last slot of a
    pass (the second), and the first slot of the last - partial or whole - pass."""
    rp, _ = x_consts(Dh)
    raw = {"pos0": 0, "last": L - 1, "pass_first": rp, "pass_last": 2 * rp - 1, "tail_first": (L - 1) // rp * rp}
    return {n: min(v, L - 1) for n, v in raw.items()}


@dataclass
class Cross:
    Dh: int
    family: str
    cap: int
    lens: np.ndarray
    q: np.ndarray                  # fp32 [rows, H, Dh]
    K: np.ndarray                  # fp32 [rows, H, cap, Dh]
    V: np.ndarray
    mask: np.ndarray
    ref: np.ndarray
    A: np.ndarray
    p: np.ndarray
    hot: np.ndarray = None


@lru_cache(maxsize=4)
def build_cross(Dh: int, family: str, seed: int = 0) -> Cross:
    rp, cap = x_consts(Dh)
    lens = x_lengths(Dh)
    rng = np.random.default_rng([seed, 13, Dh, X_FAMILIES.index(family)])
    f = np.float32
    shape = (XROWS, XH, cap, Dh)
    K, V = rng.standard_normal(shape, dtype=f), rng.standard_normal(shape, dtype=f)
    hot = None
    if family in ("random", "peaky"):
        q = rng.standard_normal((XROWS, XH, Dh), dtype=f) * f(4.0 if family == "peaky" else 1.0)
    elif family == "flat":
        q = rng.standard_normal((XROWS, XH, Dh), dtype=f)
        K = np.repeat(K[:, :, :1], cap, axis=2)
    elif family in ("ramp_up", "ramp_down"):
        # scores from 2 to 102 over the row's own len positions: the online rescale works in every pass, the slot merge across them
        sg = ac._signs(rng, (XROWS, XH, Dh))
        t = np.clip(np.arange(cap, dtype=f)[None, :] / np.maximum(lens - 1, 1)[:, None].astype(f), 0, 1)
        c = (2.0 + 100.0 * t) / np.sqrt(f(Dh))
        K = c[:, None, :, None] * sg[:, :, None, :] + K * f(0.05)
        q = sg if family == "ramp_up" else -sg
    else:
        # q = +-1: the N(0, 1) keys score N(0, 1); a needle key 8 q scores 8 sqrt(Dh) >= 45, the underflow key 24 q scores >= 135 > 104,
        # where e^-x leaves fp32: every other slot's partial vanishes against its own
        q = ac._signs(rng, (XROWS, XH, Dh))
        hot = np.zeros((XROWS, XH, 2), np.int64)
        for b in range(XROWS):
            L = int(lens[b])
            named = x_named(Dh, L)
            for h in range(XH):
                if family.startswith("needle:"):
                    hot[b, h] = named[family.split(":")[1]]
                else:
                    # two needles in different slots (lanes r = t % RP) wherever the row has two positions; the underflow key walks
                    # through the named positions
                    first = list(named.values())[(b * XH + h) % len(named)]
                    second = (first + rp // 2 + 1) % L if family == "two_needles" else first
                    hot[b, h] = first, second
                for t in set(hot[b, h].tolist()):
                    K[b, h, t] = f(24.0 if family == "underflow" else 8.0) * q[b, h]
        if family.startswith("needle:"):
            V = ac._needle_values(rng, XROWS * XH * cap, Dh).reshape(shape)
    q, K, V = ac.bf16_round(q), ac.bf16_round(K), ac.bf16_round(V)
    mask = np.arange(cap)[None, :] < lens[:, None]
    ref, A, p = ac.reference(q, K, V, mask)
    return Cross(Dh, family, cap, lens, q, K, V, mask, ref, A, p, hot)


def cross_kv(lc: Cross, outside: str = "keep") -> np.ndarray:
    """kv as the tap takes it: uint16 bf16 bits [rows, cap, 2 * H * Dh].  Positions >= len[b] hold what the launch drew ("keep"),
    "zero", "max" (the largest finite bf16, signs alternating) or "nan"."""
    kv = np.concatenate([_bits(lc.K).transpose(0, 2, 1, 3).reshape(XROWS, lc.cap, -1),
                         _bits(lc.V).transpose(0, 2, 1, 3).reshape(XROWS, lc.cap, -1)], 2)
    if outside != "keep":
        n = kv.shape[-1]
        row = {"zero": np.zeros(n, np.uint16), "nan": np.full(n, BF16_NAN, np.uint16),
               "max": np.where(np.arange(n) % 2 == 0, BF16_MAX, BF16_MAX | 0x8000).astype(np.uint16)}[outside]
        kv[~lc.mask] = row
    return np.ascontiguousarray(kv)


def run_cross(lm, lc: Cross, outside: str = "keep") -> np.ndarray:
    out = lm.debug_cross_attn(_dev(lm, _bits(lc.q)), _dev(lm, cross_kv(lc, outside)), torch.from_numpy(lc.lens))
    return ac.bf16_bits(out).reshape(XROWS, XH, lc.Dh)


def check_cross(lm, Dh: int, family: str):
    lc = build_cross(Dh, family)
    got = run_cross(lm, lc)
    if family in X_TOLERANCE:
        msg = _within(got, lc.ref, lc.A, f"cross Dh={Dh} {family}")
        assert not msg, msg
        return
    hot = lc.hot[..., 0]
    for b in range(XROWS):                     # the needle sits where its name says, restated from the length alone
        assert int(hot[b, 0]) == x_named(Dh, int(lc.lens[b]))[family.split(":")[1]] < lc.lens[b]
    want = check_needle_ref(lc.p, lc.V, hot, lc.mask)
    if not np.array_equal(got, _bits(want)):
        b, h, _ = np.argwhere(got != _bits(want))[0]
        raise AssertionError(f"cross Dh={Dh} {family}: row {b} (len {int(lc.lens[b])}) head {h}, needle on position {int(hot[b, h])}: "
                             f"{bf16_bits_to_f32(got[b, h, :4])} against {want[b, h, :4]}")


def check_cross_outside(lm, Dh: int):
    """The largest finite values, then NaN, in positions >= len[b]: bit-identical to zeros there, and finite."""
    for family in ("random", "ramp_up"):
        lc = build_cross(Dh, family)
        zero = run_cross(lm, lc, "zero")
        assert np.isfinite(bf16_bits_to_f32(zero)).all()
        for pat in ("max", "nan"):
            got = run_cross(lm, lc, pat)
            assert np.array_equal(got, zero), f"cross Dh={Dh} {family}: {pat} in positions >= len differs from zeros there, first at row " \
                                              f"{np.argwhere(got != zero)[0][0]}"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lm, lm_one=None, lm_twelve=None):
    """What the taps refuse (include/moshi_mi.h), with the status' exception and a message that names the limit."""
    import pytest
    dev = lm.device
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
    lib, h, sp = lm._lib, lm._handle, 0
    good = dict(rows=2, H=3, Dh=32, steps=8, k=3, kernel=0)

    def dep(qkv=None, kc=None, vc=None, out=None, **kw):
        a = dict(good, **kw)
        n = max(a["rows"], 1) * a["H"] * max(a["Dh"], 1)
        bufs = [z(3 * n + 8), z(n * max(a["steps"], 1) + 8), z(n * max(a["steps"], 1) + 8), z(n + 8)]
        ptr = [t.data_ptr() for t in bufs]
        for i, o in enumerate((qkv, kc, vc, out)):
            if o is not None:
                ptr[i] = o if o == 0 else ptr[i] + o
        from moshi_amd import _capi
        lib.check(lib.mmi_lm_debug_dep_attn(h, ptr[0] or None, ptr[1] or None, ptr[2] or None, a["rows"], a["H"], a["Dh"], a["steps"], a["k"],
                                            a["kernel"], ptr[3] or None, None, _capi.stream_ptr(dev)))
    dep()
    for name in ("qkv", "kc", "vc", "out"):
        with pytest.raises(ValueError, match="null argument"):
            dep(**{name: 0})
    for name in ("qkv", "kc", "vc"):
        with pytest.raises(NotImplementedError, match="16-byte aligned"):
            dep(**{name: 8})
    with pytest.raises(NotImplementedError, match="16-byte aligned, out 2-byte"):
        dep(out=1)
    for Dh in (0, 65, 72):
        with pytest.raises(NotImplementedError, match="head dim must be 1..64"):
            dep(Dh=Dh)
    for steps in (0, 33):
        with pytest.raises(AssertionError, match="steps must be 1..32"):
            dep(steps=steps, k=0)
    for k in (-1, 8):
        with pytest.raises(AssertionError, match=r"k must be in \[0, steps\)"):
            dep(k=k)
    bound = max(128, lm.max_batch)
    for rows in (0, bound + 1):
        with pytest.raises(AssertionError, match=f"rows must be 1..{bound}"):
            dep(rows=rows)
    with pytest.raises(ValueError, match="unknown kernel"):
        dep(kernel=4)
    with pytest.raises(NotImplementedError, match="multiple of 8 and steps <= 8"):
        dep(kernel=1, Dh=20)
    with pytest.raises(NotImplementedError, match="multiple of 8 and steps <= 8"):
        dep(kernel=1, steps=9)
    with pytest.raises(NotImplementedError, match="steps <= 16"):
        dep(kernel=2, steps=17)
    dep(kernel=3, steps=32, k=31)
    # ---- the cross attention
    lc = build_cross(32, "random")
    q, kv = _dev(lm, _bits(lc.q)), _dev(lm, cross_kv(lc))
    lens = torch.from_numpy(lc.lens)
    lm.debug_cross_attn(q, kv, lens)
    for bad in (0, lc.cap + 1, -3):
        wrong = lens.clone()
        wrong[5] = bad
        with pytest.raises(ValueError, match=r"every len must be in \[1, cap\]"):
            lm.debug_cross_attn(q, kv, wrong)
    with pytest.raises(NotImplementedError, match="head dim must be 32, 64 or 128"):
        lm.debug_cross_attn(q.reshape(XROWS, 4, 16), kv, lens)
    with pytest.raises(AssertionError, match=f"rows must be 1..{bound}"):
        lm.debug_cross_attn(z(bound + 1, 1, 32), z(bound + 1, 1, 64), torch.ones(bound + 1, dtype=torch.int32))
    pad = z(kv.numel() + 4)
    with pytest.raises(NotImplementedError, match="16-byte aligned"):
        lm.debug_cross_attn(q, pad[4:].reshape(kv.shape), lens)
    # ---- the attention inside out_proj: refused where the step would not fuse
    if lm_one is not None:
        cfg = lm_one.config
        dd = cfg.depformer_dim
        args = lambda: (z(3 * dd), z(dd * cfg.dep_q), z(dd * cfg.dep_q), z(dd))
        lm_one.debug_dep_attn_out_proj(0, 1, *args())
        for k in (0, cfg.dep_q):
            with pytest.raises(AssertionError, match=r"k must be in \[1, dep_q\)"):
                lm_one.debug_dep_attn_out_proj(0, k, *args())
        with pytest.raises(AssertionError, match="layer must be in"):
            lm_one.debug_dep_attn_out_proj(cfg.depformer_num_layers, 1, *args())
    if lm_twelve is not None:                  # 12 positions per frame: the step keeps the attention launch (dep_attn_fusable)
        cfg = lm_twelve.config
        dd = cfg.depformer_dim
        for fused in (True, False):
            with pytest.raises(NotImplementedError, match="dep_attn_fusable"):
                lm_twelve.debug_dep_attn_out_proj(0, 1, z(3 * dd), z(dd * cfg.dep_q), z(dd * cfg.dep_q), z(dd), fused=fused)


# ---- GAMMA -----------------------------------------------------------------------------------------------------------------------------------
def tolerance_launches():
    """Every launch the tolerance is applied to: (label, q, K, V, mask, ref, A, twin chunk)."""
    for shape in SHAPES:
        for k in shape.ks:
            for family in TOLERANCE_FAMILIES:
                lc = build_dep(shape, k, family)
                yield f"dep {shape.id} k={k} {family}", lc, 5
    for Dh in X_HEAD_DIMS:
        for family in X_TOLERANCE:
            yield f"cross Dh={Dh} {family}", build_cross(Dh, family), 37


def measure_gamma(verbose=True):
    """Worst |fp32_twin - ref| / (2^-24 A) over every tolerance launch of this list, and where."""
    worst, where = 0.0, None
    for label, lc, chunk in tolerance_launches():
        tw = ac.fp32_twin(lc.q, lc.K, lc.V, lc.mask, chunk=chunk).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.maximum(np.abs(tw - lc.ref) - ac.FLOOR, 0) / (2.0 ** -24 * lc.A)
        r = float(np.nanmax(np.where(lc.A > 0, r, 0)))
        if verbose:
            print(f"{label}: ratio {r:.2f}", flush=True)
        if r > worst:
            worst, where = r, label
    return worst, where




if __name__ == "__main__":
    w, at = measure_gamma()
    print(f"worst ratio {w:.2f} at {at}; GAMMA = 4 x that = {4 * w:.1f} (attn_cases.GAMMA = {ac.GAMMA})")
