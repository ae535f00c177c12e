"""Cases for the temporal decode attention ALONE (`mmi_lm_debug_attn` / `LMModel.debug_attn`), shared by the simulator
suite (tests/test_attn_sim.py) and the MI355X suite (tests/test_b_attn_gpu.py): k_lm_attn_wave, k_lm_attn_split, k_lm_attn_combine
and the merge by the last-arriving workgroup, on rings built so that each of their paths matters, against a softmax in fp64.

The reference (`reference`): plain numpy in fp64 on the ring bytes widened exactly (`decode`: bf16 bits, OCP e4m3 bytes, E2M1 x
E8M0).  Scores q.k / sqrt(Dh); slot s of a ring of `cap` slots holds position off + d if d = s - off % cap <= 0, else off + d - cap,
and is attended iff pos >= 0 and 0 <= off - pos < context (transformer.py:262-286, 574-582); softmax and P.V in fp64.

The tolerance, per output element d (`tolerance`):  |out - ref| <= 2^-8 |ref_d| + GAMMA 2^-24 A_d,  A_d = sum_i p_i |v_i,d|
(plus 2^-126 only where ref_d itself is below the normal range: see `tolerance`).
The first term is the one rounding to bf16 (half an ulp of bf16 is between 2^-9 and 2^-8 of the value, so a correct kernel can sit just
under 1.0 x this term alone); the second is accumulation in fp32.  GAMMA is not a guess: `measure_gamma` runs `fp32_twin` - an online softmax in
numpy fp32 that walks the ring in chunks of 37 rows, an order no kernel uses - over every launch of the case list, and GAMMA is
4 x the worst |twin - ref| / (2^-24 A_d) seen (the margin: a second summation order, expf, v_dot2).  Measured worst ratio: 50.08
(bf16, head dim 128, the rising ramp, whose scores of about 100 carry their own fp32 rounding; profiles/attn_exact/README.md) -> GAMMA = 200.3.

Every launch carries 16 sessions (rows) with an offset each, i.e. 16 ring lengths, and H = 2 heads with different data."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from tests.kv4_cases import bf16_bits_to_f32, dequantize, quantize

GAMMA = 200.3                    # 4 x 50.08, the worst ratio of fp32_twin over the case list (measure_gamma; profiles/attn_exact/README.md)
ROWS, H = 16, 2
FORMS = ("bf16", "fp8", "fp4")
HEAD_DIMS = (32, 64, 128)
CHUNK = 256                      # MMI_ATTN_CHUNK of k_lm_attn_split


@dataclass(frozen=True)
class Path:
    kernel: str                  # "wave" / "split"
    ns: int
    merge: str = "launch"        # "launch": k_lm_attn_combine; "kernel": the last-arriving workgroup, rings <= solo rows walked by workgroup 0

    @property
    def name(self):
        return f"{self.kernel}-ns{self.ns}" + ("" if self.ns == 1 else f"-{self.merge}")


# NS = 1: the early-load path of k_lm_attn_wave; NS = 3 + the combine launch; NS = 3 merged in the kernel, with solo_rows = G(1) so that
# one launch holds pairs walked by workgroup 0 alone and pairs merged by the last arriver
PATHS = (Path("wave", 1), Path("wave", 3), Path("wave", 3, "kernel"), Path("split", 1), Path("split", 3))


def consts(form: str, Dh: int, ns: int = 1):
    """(RPW, NB, G) of k_lm_attn_wave<Dh, form>: rows per wave instruction, row groups per round, rows per round of all 4 ns waves."""
    epl = {"bf16": 8, "fp8": 16, "fp4": 32}[form]
    rpw = 64 // (Dh // epl)
    nb = 2 if form == "fp4" else 4
    return rpw, nb, 4 * ns * nb * rpw


def capacity(form: str, Dh: int) -> int:
    """3 G + 5 with G of the three-workgroup split (no multiple of RPW), and no less than 517: room for the chunked kernel's 513 rows."""
    return max(3 * consts(form, Dh, 3)[2] + 5, 517)


def solo_rows(form: str, Dh: int) -> int:
    return consts(form, Dh, 1)[2]


def offset_sets(form: str, Dh: int, cap: int = None):
    """Two launches' worth of offsets.  A: the short rings, the lengths around the rounds of one workgroup, around the chunks of the
    chunked kernel.  B: the lengths around the rounds of three workgroups, cap - 1, cap, and wrapped offsets with the newest row in slot
    0, in slot cap - 1 and mid-ring.  L = offset + 1 below the wrap."""
    rpw, _, g1 = consts(form, Dh, 1)
    g3 = 3 * g1
    cap = cap or capacity(form, Dh)
    la = [1, 2, rpw - 1, rpw, rpw + 1, g1 - 1, g1, g1 + 1, 2 * g1 + 1, 3 * g1 - 1, 255, 256, 257, 513]
    lb = [g3 - 1, g3, g3 + 1, 2 * g3 + 1, 3 * g3 - 1, cap - 1, cap]
    wrapped = [cap, 2 * cap - 1, cap + cap // 2, 3 * cap, 4 * cap - 1, 2 * cap + 7, cap + 1, 5 * cap + cap // 3, cap + 2 * cap // 3]
    A = [min(max(L, 1), cap) - 1 for L in la] + wrapped[3:5]
    B = [min(L, cap) - 1 for L in lb] + wrapped
    assert len(A) == ROWS and len(B) == ROWS
    return np.array(A, np.int64), np.array(B, np.int64)


# ---- ring formats ----------------------------------------------------------------------------------------------------------------------
def _e4m3_table():
    t = np.zeros(256, np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        mag = np.nan if (e == 15 and m == 7) else (m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
        t[b] = -mag if b & 128 else mag
    return t.astype(np.float32)


E4M3 = _e4m3_table()


@dataclass
class Ring:
    """Keys or values of one launch: `codes` uint8 [rows, H, cap, bytes per row]; `scales` uint8 [rows, H, cap, Dh / 16] (4-bit) or None."""
    form: str
    codes: np.ndarray
    scales: np.ndarray = None

    def copy(self):
        return Ring(self.form, self.codes.copy(), None if self.scales is None else self.scales.copy())

    def bytes(self) -> np.ndarray:
        return self.codes.reshape(-1) if self.scales is None else np.concatenate([self.codes.reshape(-1), self.scales.reshape(-1)])

    def decode(self) -> np.ndarray:
        """fp32 [rows, H, cap, Dh], exactly what the ring holds."""
        if self.form == "bf16":
            return bf16_bits_to_f32(np.ascontiguousarray(self.codes).view(np.uint16))
        if self.form == "fp8":
            return E4M3[self.codes]
        return dequantize(self.codes, self.scales)


def encode(form: str, x: np.ndarray) -> Ring:
    """fp32 [rows, H, cap, Dh] -> the ring that holds it, rounded to the form (the tests read the values back with `decode`).  Normal
    numbers only: magnitudes are kept inside [2^-20, 2^8] (e4m3: [2^-6, 2^8]: its subnormals are out of scope); the 4-bit form also
    holds exact zeros, which its quantiser cannot avoid."""
    x = np.ascontiguousarray(x, np.float32)
    lo = 2.0 ** -6 if form == "fp8" else 2.0 ** -20
    x = np.copysign(np.clip(np.abs(x), lo, 256.0), x).astype(np.float32)
    if form == "bf16":
        bits = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        return Ring(form, np.ascontiguousarray(bits).view(np.uint8).reshape(x.shape[:-1] + (2 * x.shape[-1],)))
    if form == "fp8":
        return Ring(form, torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy())
    codes, scales = quantize(x)
    return Ring(form, codes, scales)


def bf16_round(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def valid_mask(offsets: np.ndarray, cap: int, context: int) -> np.ndarray:
    """bool [rows, cap]: the slots row b attends."""
    s = np.arange(cap, dtype=np.int64)[None, :]
    off = offsets.astype(np.int64)[:, None]
    delta = s - off % cap
    pos = np.where(delta <= 0, off + delta, off + delta - cap)
    return (pos >= 0) & (off - pos >= 0) & (off - pos < context)


def written_mask(offsets: np.ndarray, cap: int) -> np.ndarray:
    """bool [rows, cap]: the slots a stream at these offsets has ever written (slot < L)."""
    return np.arange(cap)[None, :] < np.minimum(offsets + 1, cap)[:, None]


def reference(q: np.ndarray, K: np.ndarray, V: np.ndarray, mask: np.ndarray):
    """q [rows, H, Dh], K / V [rows, H, cap, Dh] (decoded), mask [rows, cap] -> (out, A, p) in fp64: out [rows, H, Dh], A = sum p |v|."""
    q64, Dh = q.astype(np.float64), q.shape[-1]
    s = np.einsum("bhd,bhsd->bhs", q64, K.astype(np.float64)) / np.sqrt(float(Dh))
    s = np.where(mask[:, None, :], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    V64 = np.where(mask[:, None, :, None], V.astype(np.float64), 0.0)          # a masked row takes no part whatever it holds
    return np.einsum("bhs,bhsd->bhd", p, V64), np.einsum("bhs,bhsd->bhd", p, np.abs(V64)), p


FLOOR = 2.0 ** -126              # the smallest normal bf16 / fp32


def tolerance(ref: np.ndarray, A: np.ndarray) -> np.ndarray:
    """The rule; and FLOOR only where the reference itself lies below the normal range.  That happens where the attended values are a
    4-bit ring's exact zeros (or cancel exactly): the reference is then what the OTHER rows leave, weights of e^-90 and less times their
    values, about 1e-40 - a number bf16 holds only as a subnormal of a few bits (subnormal results are out of scope), while
    A_d of such an element is still 1e-37 and more."""
    return 2.0 ** -8 * np.abs(ref) + GAMMA * 2.0 ** -24 * A + np.where(np.abs(ref) < FLOOR, FLOOR, 0.0)


def fp32_twin(q: np.ndarray, K: np.ndarray, V: np.ndarray, mask: np.ndarray, chunk: int = 37) -> np.ndarray:
    """An online softmax in numpy fp32 over chunks of 37 slots (no kernel's order): what fp32 accumulation costs, for GAMMA."""
    f = np.float32
    rows, Hh, cap, Dh = K.shape
    m = np.full((rows, Hh), -np.inf, f)
    l = np.zeros((rows, Hh), f)
    acc = np.zeros((rows, Hh, Dh), f)
    scale = f(1.0) / np.sqrt(f(Dh))
    with np.errstate(invalid="ignore"):
        for c0 in range(0, cap, chunk):
            sl = slice(c0, min(c0 + chunk, cap))
            s = np.einsum("bhd,bhsd->bhs", q.astype(f), K[:, :, sl].astype(f)).astype(f) * scale
            s = np.where(mask[:, None, sl], s, f(-np.inf))
            mn = np.maximum(m, s.max(-1))
            live = mn > -np.inf
            resc = np.where(live & (m > -np.inf), np.exp(np.where(live, m - mn, 0).astype(f)), f(0)).astype(f)
            p = np.where(live[..., None], np.exp(np.where(live[..., None], s - mn[..., None], -np.inf).astype(f)), f(0)).astype(f)
            Vc = np.where(mask[:, None, sl, None], V[:, :, sl].astype(f), f(0))
            l = (l * resc + p.sum(-1, dtype=f)).astype(f)
            acc = (acc * resc[..., None] + np.einsum("bhs,bhsd->bhd", p, Vc).astype(f)).astype(f)
            m = mn
    return (acc / l[..., None]).astype(f)


# ---- input families -------------------------------------------------------------------------------------------------------------------------
@dataclass
class Launch:
    """One launch of one family: operands as the tap takes them, and what the reference says about them."""
    form: str
    Dh: int
    cap: int
    context: int
    offsets: np.ndarray
    q: np.ndarray               # fp32 [rows, H, Dh], bf16 values
    K: Ring
    V: Ring
    mask: np.ndarray
    ref: np.ndarray = None      # fp64 [rows, H, Dh]
    A: np.ndarray = None
    p: np.ndarray = None        # fp64 [rows, H, cap]
    note: dict = None
    Kd: np.ndarray = None       # the rings decoded, fp32 [rows, H, cap, Dh]
    Vd: np.ndarray = None


def _signs(rng, shape):
    return rng.integers(0, 2, shape).astype(np.float32) * 2 - 1


def wave_slot(form, Dh, ns, y, w, j, r=0):
    """Slot of row r of the j-th row group of wave w of workgroup y of k_lm_attn_wave (row groups dealt round-robin over all waves)."""
    rpw = consts(form, Dh)[0]
    return ((y * 4 + w) + j * 4 * ns) * rpw + r


def needle_slots(form: str, Dh: int, off: int, cap: int):
    """Where a needle is put for a ring at offset `off`: slot 0, L - 1, the newest row (end_index), the oldest (end_index + 1), first
    and last row of a row group, of a round (one and three workgroups) and of a 256 chunk, and one slot in each workgroup's share of
    both kernels at NS = 3 (wave: every wave of every workgroup; chunked: chunk c belongs to workgroup c % 3)."""
    rpw, _, g1 = consts(form, Dh, 1)
    L, end = min(off + 1, cap), off % cap
    s = [0, L - 1, end, (end + 1) % cap, rpw, 2 * rpw - 1, g1, 2 * g1 - 1, 3 * g1, 6 * g1 - 1, 255, 256, 511, 512]
    s += [wave_slot(form, Dh, 3, y, w, 1, 1) for y in range(3) for w in range(4)]
    s += [wave_slot(form, Dh, 1, 0, w, 2, rpw - 1) for w in range(4)]
    s += [CHUNK * c + 7 + 64 * (c % 4) for c in range(6)]
    out = []
    for x in s:
        x = min(max(int(x), 0), L - 1)
        if x not in out:
            out.append(x)
    return out


NAMED = ("slot0", "last", "newest", "oldest", "group_first", "group_last", "round1_first", "round1_last", "round3_first", "round3_last",
         "chunk_last", "chunk_first", "chunk2_last", "chunk2_first")


def named_slots(form: str, Dh: int, off: int, cap: int) -> dict:
    """The positions the needle is put on DELIBERATELY, on every ring of a launch: slot 0, L - 1, the newest row (end_index = off % cap),
    the oldest row (end_index + 1 once the ring has wrapped, slot 0 before), first and last row of a row group, of a round of one and of
    three workgroups, of a 256 chunk.  Clamped to L - 1 on rings too short to have them."""
    rpw, _, g1 = consts(form, Dh, 1)
    L, end = min(off + 1, cap), off % cap
    raw = (0, L - 1, end, (end + 1) % cap if off + 1 >= cap else 0, rpw, 2 * rpw - 1, g1, 2 * g1 - 1, 3 * g1, 6 * g1 - 1, 255, 256, 511, 512)
    return {n: min(int(x), L - 1) for n, x in zip(NAMED, raw)}


def share_slots(form: str, Dh: int, off: int, cap: int):
    """One slot in each workgroup's share of both kernels at NS = 3 (wave: every wave of every workgroup; chunked: chunk c belongs to
    workgroup c % 3) and in every wave's share at NS = 1, clamped to L - 1."""
    rpw = consts(form, Dh, 1)[0]
    L = min(off + 1, cap)
    s = [wave_slot(form, Dh, 3, y, w, 1, 1) for y in range(3) for w in range(4)]
    s += [wave_slot(form, Dh, 1, 0, w, 2, rpw - 1) for w in range(4)]
    s += [CHUNK * c + 7 + 64 * (c % 4) for c in range(6)]
    out = []
    for x in s:
        x = min(int(x), L - 1)
        if x not in out:
            out.append(x)
    return out


def _needle_values(rng, n, Dh):
    """Value rows without a zero (a 4-bit ring rounds small elements to exact zeros, where the output would be the e^-40 the other rows
    leave instead of V[j]): +-{1, 1.5, 2, 3, 4, 6}, which every form holds exactly."""
    return np.array([1, 1.5, 2, 3, 4, 6], np.float32)[rng.integers(0, 6, (n, Dh))] * _signs(rng, (n, Dh))


@lru_cache(maxsize=2)
def base_rings(form: str, Dh: int, cap: int, seed: int = 0):
    """The N(0, 1) key and value rings that every family of one (form, head dim) starts from, with their decoded values: encoded once
    (the families patch a few rows or bring a query of their own).  Read-only."""
    rng = np.random.default_rng([seed, FORMS.index(form), Dh, cap])
    shape = (ROWS, H, cap, Dh)
    K, V = encode(form, rng.standard_normal(shape, dtype=np.float32)), encode(form, rng.standard_normal(shape, dtype=np.float32))
    return K, V, K.decode(), V.decode()


@lru_cache(maxsize=1)
def ramp_keys(form: str, Dh: int, cap: int, seed: int = 0):
    """Keys whose scores against q = sign pattern `sg` rise along the slots by about 100 over the written part of set B's rings:
    key i = c_i sg + noise, score c_i sqrt(Dh) from 2 to 102."""
    rng = np.random.default_rng([seed, 7, FORMS.index(form), Dh, cap])
    offsets = offset_sets(form, Dh, cap)[1]
    sg = _signs(rng, (ROWS, H, Dh))
    Lr = np.minimum(offsets + 1, cap)
    t = np.clip(np.arange(cap, dtype=np.float32)[None, :] / np.maximum(Lr - 1, 1)[:, None].astype(np.float32), 0, 1)   # 0 .. 1 over slots < L
    c = (2.0 + 100.0 * t) / np.sqrt(np.float32(Dh))
    K = encode(form, c[:, None, :, None] * sg[:, :, None, :] + rng.standard_normal((ROWS, H, cap, Dh), dtype=np.float32) * np.float32(0.05))
    return sg, K, K.decode()


def _patched(form, ring: Ring, dec: np.ndarray, where, rows: np.ndarray):
    """Copies of (ring, decoded values) with the slots where = [(b, h, slot)] holding rows [n, Dh]."""
    ring, dec = ring.copy(), dec.copy()
    if len(where):
        small = encode(form, rows[None, None])
        b, h, s = (np.array(x) for x in zip(*where))
        ring.codes[b, h, s] = small.codes[0, 0]
        if ring.scales is not None:
            ring.scales[b, h, s] = small.scales[0, 0]
        dec[b, h, s] = small.decode()[0, 0]
    return ring, dec


def build(form: str, Dh: int, family: str, which: str = "B", seed: int = 0, cap: int = None) -> Launch:
    """The launch of `family` at offset set `which` ("A" / "B", offset_sets)."""
    cap = cap or capacity(form, Dh)
    # a seed of the case's own (a tuple hash is per-process in Python)
    rng = np.random.default_rng([seed, FORMS.index(form), Dh, sum(map(ord, family)), ord(which[0])])
    offsets = offset_sets(form, Dh, cap)[0 if which == "A" else 1]
    K, V, Kd, Vd = base_rings(form, Dh, cap, seed)
    context, note = cap, {}
    if family in ("random", "flat", "peaky"):
        q = rng.standard_normal((ROWS, H, Dh), dtype=np.float32) * np.float32({"random": 1.0, "flat": 1.0 / 16, "peaky": 4.0}[family])
    elif family.startswith("needle:"):
        # ONE needle per (row, head), bit for bit.  "needle:k", k = 0 .. 6: head h of EVERY ring carries the named position 2 k + h
        # (NAMED) - so slot 0, L - 1, the newest and the oldest row and every edge are hit on wrapped and on unwrapped rings alike;
        # "needle:shares": the pairs walk through share_slots.  q = +-1: the N(0, 1) keys score N(0, 1), the needle key 8 q scores
        # 8 sqrt(Dh) >= 45
        kind = family.split(":")[1]
        q = _signs(rng, (ROWS, H, Dh))
        hot = np.zeros((ROWS, H, 2), np.int64)
        names = [[None] * H for _ in range(ROWS)]
        where = []
        for b in range(ROWS):
            off = int(offsets[b])
            for h in range(H):
                if kind == "shares":
                    slots = share_slots(form, Dh, off, cap)
                    names[b][h], hot[b, h] = "share", slots[(b * H + h) % len(slots)]
                else:
                    names[b][h] = NAMED[2 * int(kind) + h]
                    hot[b, h] = named_slots(form, Dh, off, cap)[names[b][h]]
                where.append((b, h, int(hot[b, h, 0])))
        K, Kd = _patched(form, K, Kd, where, np.array([8.0 * q[b, h] for b, h, _ in where], np.float32))
        V, Vd = _patched(form, V, Vd, where, _needle_values(rng, len(where), Dh))
        note.update(hot=hot, names=names)
    elif family == "wneedle":
        # context < cap, bit for bit - the sharp check of the slot map, which the kernels consult only under a window.  Head 0: the needle
        # sits on the OLDEST position inside the window (position 0 while the stream is shorter), and the position just outside it,
        # which the mask must drop, holds a decoy twice as strong.  Head 1: the needle sits on the newest row (end_index), same decoy.
        context = max(cap // 3, 2)
        q = _signs(rng, (ROWS, H, Dh))
        hot = np.zeros((ROWS, H, 2), np.int64)
        names = [["window_oldest", "window_newest"] for _ in range(ROWS)]
        where, decoys = [], []
        for b in range(ROWS):
            off = int(offsets[b])
            oldest = max(off - context + 1, 0)
            for h, pos in enumerate((oldest, off)):
                hot[b, h] = pos % cap
                where.append((b, h, pos % cap))
                if oldest - 1 >= 0 and off - (oldest - 1) < cap:
                    decoys.append((b, h, (oldest - 1) % cap))
        K, Kd = _patched(form, K, Kd, where + decoys, np.array([8.0 * q[b, h] for b, h, _ in where] + [16.0 * q[b, h] for b, h, _ in decoys], np.float32))
        V, Vd = _patched(form, V, Vd, where, _needle_values(rng, len(where), Dh))
        note.update(hot=hot, names=names, decoys=decoys)
    elif family in ("two_needles", "underflow"):
        # (under the tolerance rule) q = +-1 in every element: the N(0, 1) keys score N(0, 1).  The needle key 8 q scores 8 sqrt(Dh) >= 45;
        # the underflow key 24 q scores 24 sqrt(Dh) >= 135 > 104, where e^-x leaves fp32: every other wave's and workgroup's partial vanishes against its own
        q = _signs(rng, (ROWS, H, Dh))
        hot = np.zeros((ROWS, H, 2), np.int64)
        where, rows = [], []
        for b in range(ROWS):
            slots = needle_slots(form, Dh, int(offsets[b]), cap)
            for h in range(H):
                i = (b * H + h) % len(slots)
                hot[b, h] = slots[i], (slots[(i + len(slots) // 2) % len(slots)] if family == "two_needles" else slots[i])
                for j in sorted(set(hot[b, h].tolist())):
                    where.append((b, h, j))
                    rows.append((24.0 if family == "underflow" else 8.0) * q[b, h])
        K, Kd = _patched(form, K, Kd, where, np.array(rows, np.float32))
        note["hot"] = hot
    elif family in ("ramp_up", "ramp_down"):
        # ramp_down: the same keys under -q, scores from -2 down to -102
        sg, K, Kd = ramp_keys(form, Dh, cap, seed)
        q = sg if family == "ramp_up" else -sg
    elif family == "windowed":
        # context < cap: offsets before and after the wrap.  The oldest position inside the window carries a needle, the position just
        # outside it (masked) a decoy twice as strong, the newest row a second needle - under the tolerance rule
        context = max(cap // 3, 2)
        q = _signs(rng, (ROWS, H, Dh))
        where, rows = [], []
        for b in range(ROWS):
            off = int(offsets[b])
            for pos, amp in ((off - context + 1, 8.0), (off - context, 16.0), (off, 8.0)):
                if pos >= 0 and off - pos < cap and not any(w[0] == b and w[2] == pos % cap for w in where):
                    for h in range(H):
                        where.append((b, h, pos % cap))
                        rows.append(amp * q[b, h])
        K, Kd = _patched(form, K, Kd, where, np.array(rows, np.float32))
    else:
        raise KeyError(family)
    q = bf16_round(q)
    mask = valid_mask(offsets, cap, context)
    ref, A, p = reference(q, Kd, Vd, mask)
    return Launch(form, Dh, cap, context, offsets, q, K, V, mask, ref, A, p, note, Kd, Vd)


NEEDLES = tuple((f"needle:{k}", "B") for k in range(7)) + (("needle:shares", "B"), ("needle:0", "A"), ("needle:1", "A"), ("needle:shares", "A"),
                                                            ("wneedle", "B"), ("wneedle", "A"))
FAMILIES = (("random", "A"), ("random", "B"), ("flat", "A"), ("peaky", "B")) + NEEDLES + (
    ("two_needles", "B"), ("underflow", "B"), ("ramp_up", "B"), ("ramp_down", "B"), ("windowed", "B"), ("windowed", "A"))


cached_build = lru_cache(maxsize=3)(build)


# ---- garbage and NaN outside the attended part -----------------------------------------------------------------------------------------
def fill_rows(ring: Ring, rows_mask: np.ndarray, pattern: str, finite_scale: bool = False) -> Ring:
    """A copy of `ring` whose slots rows_mask [rows, cap] hold `pattern` in every head: "zero"; "garbage" = the largest finite value of
    the form, signs alternating (bf16 +-3.39e38, e4m3 +-448, 4-bit code 6 under scale byte 254 - or 252 with finite_scale, see
    check_garbage); "nan" (bf16 0x7fc0, e4m3 0x7f, 4-bit scale byte 0xff)."""
    out = ring.copy()
    m = np.broadcast_to(rows_mask[:, None, :], out.codes.shape[:3])
    n = out.codes.shape[-1]
    if pattern == "zero":
        row, sc = np.zeros(n, np.uint8), 0
    elif ring.form == "bf16":
        row = np.tile(np.array([0x7f, 0x7f, 0x7f, 0xff] if pattern == "garbage" else [0xc0, 0x7f, 0xc0, 0x7f], np.uint8), n // 4)
        sc = 0
    elif ring.form == "fp8":
        row = np.tile(np.array([0x7e, 0xfe] if pattern == "garbage" else [0x7f, 0x7f], np.uint8), n // 2)
        sc = 0
    else:
        row = np.full(n, 0xe6, np.uint8)               # +6 in the low nibble, -6 in the high one
        sc = (252 if finite_scale else 254) if pattern == "garbage" else 0xff
    out.codes[m] = row
    if out.scales is not None:
        out.scales[m] = sc
    return out


# ---- running the tap ------------------------------------------------------------------------------------------------------------------
STATS: dict = {}                 # (kernel, form, Dh) -> worst |out - ref| / tolerance seen in this process


def _dump_stats():
    path = os.environ.get("MMI_ATTN_STATS")
    if path and STATS:
        with open(path, "w") as f:
            json.dump({"|".join(map(str, k)): v for k, v in sorted(STATS.items())}, f, indent=1)


def run(lm, lc: Launch, path: Path, K: Ring = None, V: Ring = None) -> np.ndarray:
    """The tap on a launch -> bf16 bits uint16 [rows, H, Dh]."""
    dev = lm.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = lm.debug_attn(t(lc.q).to(torch.bfloat16), t((K or lc.K).bytes()), t((V or lc.V).bytes()), t(lc.offsets), cap=lc.cap,
                        context=lc.context, ring=lc.form, kernel=path.kernel, ns=path.ns, merge=path.merge,
                        solo_rows=solo_rows(lc.form, lc.Dh) if path.merge == "kernel" else -1)
    return bf16_bits(out).reshape(ROWS, H, lc.Dh)


def check_tolerance(lm, lc: Launch, paths=PATHS, label=""):
    bad = []
    tol = tolerance(lc.ref, lc.A)
    for path in paths:
        got = bf16_bits_to_f32(run(lm, lc, path)).astype(np.float64)
        with np.errstate(invalid="ignore"):
            ratio = np.abs(got - lc.ref) / tol
        ratio = np.where(np.isfinite(got), ratio, np.inf)
        worst = float(ratio.max())
        key = (path.kernel, lc.form, lc.Dh)
        STATS[key] = max(STATS.get(key, 0.0), worst)
        print(f"{label} {lc.form} Dh={lc.Dh} {path.name}: worst |out - ref| / tolerance = {worst:.3f}")
        if not worst <= 1.0:
            b, h, d = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            bad.append(f"{path.name}: {worst:.3g} x the tolerance at row {b} (offset {int(lc.offsets[b])}) head {h} dim {d}: "
                       f"{got[b, h, d]!r} against {lc.ref[b, h, d]!r}; {int((ratio > 1).sum())} elements out")
    _dump_stats()
    assert not bad, f"{label} {lc.form} Dh={lc.Dh} cap={lc.cap}: " + " | ".join(bad)


def check_needle_placement(lc: Launch):
    """The needle of every (row, head) sits where its name says, restated from the offset alone - on wrapped rings the newest row is
    slot off % cap and the oldest the slot after it, wherever those fall."""
    rpw, _, g1 = consts(lc.form, lc.Dh, 1)
    edges = dict(group_first=rpw, group_last=2 * rpw - 1, round1_first=g1, round1_last=2 * g1 - 1, round3_first=3 * g1,
                 round3_last=6 * g1 - 1, chunk_last=255, chunk_first=256, chunk2_last=511, chunk2_first=512)
    for b in range(ROWS):
        off, cap = int(lc.offsets[b]), lc.cap
        wrapped, L = off + 1 >= cap, min(off + 1, cap)
        for h in range(H):
            name, slot = lc.note["names"][b][h], int(lc.note["hot"][b, h, 0])
            assert 0 <= slot < L and lc.mask[b, slot], (name, b, h, slot)
            if name == "slot0":
                assert slot == 0
            elif name == "last":
                assert slot == L - 1
            elif name in ("newest", "window_newest"):
                assert slot == off % cap
            elif name == "oldest":
                assert slot == ((off + 1) % cap if wrapped else 0)
            elif name == "window_oldest":
                want = max(off - lc.context + 1, 0)                      # a position; it lives in slot position % cap
                assert slot == want % cap and lc.context < cap
                if want > 0:                                              # the decoy one position further back is in the ring, and masked
                    assert (b, h, (want - 1) % cap) in lc.note["decoys"] and not lc.mask[b, (want - 1) % cap]
            elif name in edges:
                assert slot == min(edges[name], L - 1)
            else:
                assert name == "share"


def check_needle(lm, lc: Launch, paths=PATHS):
    """The output is V[needle] bit for bit (widened: bf16 holds every e4m3 and every 4-bit ring value exactly)."""
    hot = lc.note["hot"][..., 0]
    check_needle_placement(lc)
    bi, hi = np.meshgrid(np.arange(ROWS), np.arange(H), indexing="ij")
    w = lc.p[bi, hi, hot]
    assert (w >= 1 - 2.0 ** -30).all(), f"the reference gives a needle only {w.min()!r}"
    Vd = lc.Vd
    want = Vd[bi, hi, hot]
    for b in range(ROWS):                         # no other written row holds the needle's values: a wrong slot is a wrong answer
        L = int(min(lc.offsets[b] + 1, lc.cap))
        for h in range(H):
            assert int((Vd[b, h, :L] == want[b, h]).all(-1).sum()) == 1
    assert np.array_equal(bf16_round(want), want)
    want_bits = (want.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    bad = []
    for path in paths:
        got = run(lm, lc, path)
        if not np.array_equal(got, want_bits):
            b, h, _ = np.argwhere(got != want_bits)[0]
            bad.append(f"{path.name}: row {b} (offset {int(lc.offsets[b])}) head {h}, needle in slot {int(hot[b, h])}: "
                       f"{bf16_bits_to_f32(got[b, h, :4])} against {want[b, h, :4]}; {int((got != want_bits).any(-1).sum())} pairs differ")
    assert not bad, f"needle {lc.form} Dh={lc.Dh} cap={lc.cap}: " + " | ".join(bad)


def check_outside(lm, lc: Launch, pattern: str, paths=PATHS):
    """Whatever the slots hold that a row does not attend - never written (slot >= L) or, under a window, masked out - the result equals
    the run on zeros there bit for bit, and is finite.

    "garbage", 4-bit ring: code 6 under scale byte 254 is 6 * 2^127 - above what fp32, into which the kernels widen, can hold, so it
    reads as Inf.  It is what never-written slots get here (slot >= L: no kernel may use what it loaded from there at all).  A slot
    that is written but masked by the window is used as p * v with p = 0, in these kernels as in the reference's softmax(masked) @ V,
    which needs a finite v: those slots get the largest 4-bit value fp32 holds, code 6 under scale byte 252 = 1.5 * 2^127."""
    never = ~written_mask(lc.offsets, lc.cap)
    masked = ~lc.mask & ~never
    rings = {}
    for pat in ("zero", pattern):
        kv = []
        for ring in (lc.K, lc.V):
            r = fill_rows(ring, never, pat)
            if pattern == "garbage":              # NaN goes to never-written slots only
                r = fill_rows(r, masked, pat, finite_scale=True)
            kv.append(r)
        rings[pat] = kv
    if pattern == "nan":
        with np.errstate(over="ignore", invalid="ignore"):            # the poison decodes to NaN (4-bit: to NaN or Inf) everywhere
            assert not np.isfinite(rings[pattern][1].decode()[np.broadcast_to(never[:, None, :], (ROWS, H, lc.cap))]).any()
    bad = []
    for path in paths:
        zero = run(lm, lc, path, *rings["zero"])
        got = run(lm, lc, path, *rings[pattern])
        if not np.isfinite(bf16_bits_to_f32(got)).all():
            bad.append(f"{path.name}: {int((~np.isfinite(bf16_bits_to_f32(got))).any((1, 2)).sum())} rows are not finite")
        elif not np.array_equal(got, zero):
            b = np.argwhere(got != zero)[0][0]
            bad.append(f"{path.name}: differs from the zero-filled run, first at row {b} (offset {int(lc.offsets[b])})")
    assert not bad, f"{pattern} outside the attended part, {lc.form} Dh={lc.Dh} cap={lc.cap} context={lc.context}: " + " | ".join(bad)


GRID = [(form, Dh, family, which) for form in FORMS for Dh in HEAD_DIMS for family, which in FAMILIES]       # (form, head dim) outermost:
OUTSIDE = [(form, Dh, family, which) for form in FORMS for Dh in HEAD_DIMS                                   # base_rings is built once each
           for family, which in (("random", "A"), ("random", "B"), ("windowed", "A"), ("windowed", "B"))]


def check_family(lm, form, Dh, family, which, paths=PATHS, cap=None):
    lc = cached_build(form, Dh, family, which, 0, cap)
    if family.startswith("needle:") or family == "wneedle":
        check_needle(lm, lc, paths)
    else:
        check_tolerance(lm, lc, paths, label=f"{family}/{which}")


def check_refusals(lm):
    """What the tap refuses (include/moshi_mi.h)."""
    import pytest
    lc = build("bf16", 32, "random", "A", cap=40)
    dev = lm.device
    q = torch.from_numpy(lc.q).to(torch.bfloat16).to(dev)
    k, v, off = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (lc.K.bytes(), lc.V.bytes(), lc.offsets))
    lm.debug_attn(q, k, v, off, cap=40)
    with pytest.raises(NotImplementedError, match="head dim"):
        lm.debug_attn(q.reshape(ROWS, H * 2, 16), k, v, off, cap=40)
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        lm.debug_attn(q.reshape(ROWS, H * 2, 16), torch.zeros(ROWS * H * 2 * 40 * 9, dtype=torch.uint8, device=dev),
                      torch.zeros(ROWS * H * 2 * 40 * 9, dtype=torch.uint8, device=dev), off, cap=40, ring="fp4")
    with pytest.raises(AssertionError, match="max_batch"):
        big = lm.max_batch + 1
        lm.debug_attn(torch.zeros(big, 1, 32), torch.zeros(big * 64, dtype=torch.uint8), torch.zeros(big * 64, dtype=torch.uint8),
                      torch.zeros(big, dtype=torch.int64), cap=1)
    with pytest.raises(AssertionError, match="context"):
        lm.debug_attn(q, k, v, off, cap=40, context=41)
    with pytest.raises(AssertionError, match="NS"):
        lm.debug_attn(q, k, v, off, cap=40, ns=17)
    with pytest.raises(NotImplementedError, match="merges its partials itself"):
        lm.debug_attn(q, k, v, off, cap=40, kernel="split", ns=3, merge="kernel")
    with pytest.raises(ValueError, match="negative offset"):
        lm.debug_attn(q, k, v, off - 1, cap=40)
    pad = torch.zeros(k.numel() + 8, dtype=torch.uint8, device=dev)          # a ring 8 bytes off a 16-byte boundary
    pad[8:] = k
    with pytest.raises(NotImplementedError, match="aligned"):
        lm.debug_attn(q, pad[8:], v, off, cap=40)


# ---- GAMMA --------------------------------------------------------------------------------------------------------------------------------
def measure_gamma(verbose=True):
    """Worst |fp32_twin - ref| / (2^-24 A) over every launch of the case list: GAMMA = 4 x this."""
    worst = {}
    for form in FORMS:
        for Dh in HEAD_DIMS:
            for family, which in FAMILIES:
                lc = build(form, Dh, family, which)
                tw = fp32_twin(lc.q, lc.Kd, lc.Vd, lc.mask).astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    r = np.maximum(np.abs(tw - lc.ref) - FLOOR, 0) / (2.0 ** -24 * lc.A)
                r = float(np.nanmax(np.where(lc.A > 0, r, 0)))
                frac = float((np.abs(tw - lc.ref) / tolerance(lc.ref, lc.A)).max())
                worst[(form, Dh, family, which)] = (r, frac)
                if verbose:
                    print(f"{form} Dh={Dh} {family}/{which} cap={lc.cap}: ratio {r:.2f}, twin at {frac:.3f} x the tolerance", flush=True)
    return worst


if __name__ == "__main__":
    w = measure_gamma()
    k = max(w, key=lambda c: w[c][0])
    print(f"worst ratio {w[k][0]:.2f} at {k}; GAMMA = 4 x that = {4 * w[k][0]:.1f}; twin at most {max(v[1] for v in w.values()):.3f} x the tolerance")
