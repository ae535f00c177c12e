"""Cases for chunked prefill (`mmi_lm_prefill` / `LMGen.prefill`), shared by the simulator suite
(tests/test_prefill_sim.py) and the MI355X suite (tests/test_b_prefill_gpu.py).

Part A holds the new attention kernel ALONE (`LMModel.debug_prefill_attn`: k_lm_attn_prefill through the launch function of a pass)
to the fp64 softmax of tests/attn_cases.py - `encode`, `reference`, `valid_mask`, `tolerance` are used unchanged.  A launch is one or
two sessions' blocks of query rows; what a block attends - the ring as a stream standing at the block's start holds it, then the
block itself - is also laid out as one VIRTUAL ring without a wrap (positions base .. p0 + F - 1, base = max(0, p0 - cap): every
position the window of any of the block's queries can reach), on which `valid_mask` states the rule (pos >= 0 and
0 <= p - pos < context) and `reference` the answer.

GAMMA: `measure_gamma` runs `attn_cases.fp32_twin` (numpy fp32 online softmax in chunks of 37, no kernel's order) over every
tolerance launch of this list; 4 x the worst ratio is 4 x 27.59 = 110.3 (bf16, head dim 128, peaky, two sessions of 64 rows;
profiles/prefill/README.md), below attn_cases.GAMMA = 200.3 - so the tolerance is attn_cases.tolerance as it stands.

Part B holds the call to its definition: equality with forced steps under an exec mask of exactly the named sessions."""
from __future__ import annotations

from dataclasses import dataclass, replace
from functools import lru_cache

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config, tiny_stt_config
from moshi_amd.lm import LMGen, LMModel, SessionSampling
from oracle.lm_oracle import LMOracle
from tests import attn_cases as ac
from tests import lm_cases as lc
from tests.kv4_cases import bf16_bits_to_f32
from tests.lm_cases import cached_lm_state_dict

KT = 32                           # MMI_PF_QT: query rows of a tile = key rows of a tile of k_lm_attn_prefill
H = 2
CAP = 3 * KT + 5                  # 101: no multiple of the key tile
GAMMA_MEASURED = 110.3            # 4 x 27.59 (measure_gamma); <= attn_cases.GAMMA, which therefore stays the tolerance's
assert GAMMA_MEASURED <= ac.GAMMA


@dataclass(frozen=True)
class Shape:
    """Blocks of F rows; session i starts at position starts[i]."""
    name: str
    F: int
    starts: tuple
    context: int = CAP


# block sizes 1, 31, 32, 33, 128 of one session and two sessions sharing a launch; rings empty, shorter than the block, cap - 1,
# cap, wrapped with the block straddling slot cap - 1 -> 0; one window shorter than the ring
SHAPES = (
    Shape("1row-empty", 1, (0,)),
    Shape("31rows-cap-1", 31, (CAP - 1,)),
    Shape("32rows-cap", 32, (CAP,)),
    Shape("33rows-short-ring", 33, (7,)),
    Shape("128rows-empty", 128, (0,)),
    Shape("128rows-wrapped", 128, (3 * CAP - 40,)),
    Shape("2x64rows", 64, (5, 4 * CAP - 20)),
    Shape("128rows-window", 128, (CAP + 9,), context=CAP // 3),
)
TOL_FAMILIES = ("random", "flat", "peaky")
NEEDLES = ("oldest_first", "oldest_last", "newest_ring", "first_staged", "last_staged", "own", "future_decoy")


@dataclass
class Launch:
    form: str
    Dh: int
    shape: Shape
    q: np.ndarray                 # fp32 [rows, H, Dh], bf16 values
    row_ring: np.ndarray          # int32 [rows]
    row_pos: np.ndarray           # int64 [rows]
    k_ring: np.ndarray            # uint8: [n, H, cap, row bytes] (+ scale plane)
    v_ring: np.ndarray
    k_staged: np.ndarray          # uint8: [rows, H, row bytes] (+ scale bytes)
    v_staged: np.ndarray
    Kd: np.ndarray                # the virtual rings decoded, fp32 [rows, H, capv, Dh]
    Vd: np.ndarray
    mask: np.ndarray              # bool [rows, capv]
    ref: np.ndarray
    A: np.ndarray
    p: np.ndarray
    vidx: dict                    # (session, position) -> index into the virtual ring
    note: dict


def _virtual(shape: Shape):
    """Per session: (base, Lr) - first position the ring still holds and how many it holds; the virtual ring is Lr + F long."""
    return [(max(0, p0 - CAP), min(p0, CAP)) for p0 in shape.starts]


def _planes(ring: ac.Ring, order=None):
    """uint8 bytes of a Ring whose leading axes are transposed by `order`: the codes plane, then the scale plane."""
    c = ring.codes if order is None else ring.codes.transpose(order)
    out = [np.ascontiguousarray(c).reshape(-1)]
    if ring.scales is not None:
        s = ring.scales if order is None else ring.scales.transpose(order)
        out.append(np.ascontiguousarray(s).reshape(-1))
    return np.concatenate(out)


def _assemble(form, Dh, shape: Shape, q, Kv: list, Vv: list, note, never=None, staged_fill=None) -> Launch:
    """Kv / Vv: per session fp32 [H, Lr + F, Dh] values of the virtual ring.  never: what the ring's never-written slots hold
    ("zero" / "garbage" / "nan"); staged_fill = (pattern, j0): the staged rows >= j0 of every block hold that instead of their values."""
    n, F, cap = len(shape.starts), shape.F, CAP
    virt = _virtual(shape)
    capv = max(Lr for _, Lr in virt) + F
    rows = n * F
    ring_k, ring_v, st_k, st_v = [], [], [], []
    Kd = np.zeros((n, H, capv, Dh), np.float32)
    Vd = np.zeros((n, H, capv, Dh), np.float32)
    vidx = {}
    for i, (p0, (base, Lr)) in enumerate(zip(shape.starts, virt)):
        for src, dec, rings, staged in ((Kv[i], Kd, ring_k, st_k), (Vv[i], Vd, ring_v, st_v)):
            enc = ac.encode(form, src[None])                        # [1, H, Lr + F, .]
            dec[i, :, :Lr + F] = enc.decode()[0]
            phys = ac.encode(form, np.ones((1, H, cap, Dh), np.float32))
            phys.codes[:] = 0
            if phys.scales is not None:
                phys.scales[:] = 0
            slots = (base + np.arange(Lr)) % cap
            phys.codes[0][:, slots] = enc.codes[0][:, :Lr]
            if phys.scales is not None:
                phys.scales[0][:, slots] = enc.scales[0][:, :Lr]
            if never is not None:
                phys = ac.fill_rows(phys, (np.arange(cap) >= Lr)[None, :], never)
            blockr = ac.Ring(form, enc.codes[:, :, Lr:].copy(), None if enc.scales is None else enc.scales[:, :, Lr:].copy())
            if staged_fill is not None:
                blockr = ac.fill_rows(blockr, (np.arange(F) >= staged_fill[1])[None, :], staged_fill[0], finite_scale=True)
            rings.append(phys)
            staged.append(blockr)
        for v in range(Lr + F):
            vidx[(i, base + v)] = v

    def cat(rs):
        return ac.Ring(form, np.concatenate([r.codes for r in rs]), None if rs[0].scales is None else np.concatenate([r.scales for r in rs]))
    row_ring = np.repeat(np.arange(n, dtype=np.int32), F)
    row_pos = np.concatenate([p0 + np.arange(F, dtype=np.int64) for p0 in shape.starts])
    off_v = np.concatenate([p0 - base + np.arange(F, dtype=np.int64) for p0, (base, _) in zip(shape.starts, virt)])
    mask = ac.valid_mask(off_v, capv, shape.context)
    q = ac.bf16_round(q)
    ref, A, p = ac.reference(q, Kd[row_ring], Vd[row_ring], mask)
    return Launch(form, Dh, shape, q, row_ring, row_pos, _planes(cat(ring_k)), _planes(cat(ring_v)), _planes(cat(st_k), (0, 2, 1, 3)),
                  _planes(cat(st_v), (0, 2, 1, 3)), Kd[row_ring], Vd[row_ring], mask, ref, A, p, vidx, note)


def _rng(form, Dh, shape, family):
    return np.random.default_rng([ac.FORMS.index(form), Dh, sum(map(ord, shape.name)), sum(map(ord, family))])


@lru_cache(maxsize=4)
def build(form: str, Dh: int, shape: Shape, family: str, never=None, staged_fill=None) -> Launch:
    rng = _rng(form, Dh, shape, family)
    n, F = len(shape.starts), shape.F
    virt = _virtual(shape)
    Kv = [rng.standard_normal((H, Lr + F, Dh), dtype=np.float32) for _, Lr in virt]
    Vv = [rng.standard_normal((H, Lr + F, Dh), dtype=np.float32) for _, Lr in virt]
    note = {}
    if family in TOL_FAMILIES:
        q = rng.standard_normal((n * F, H, Dh), dtype=np.float32) * np.float32({"random": 1.0, "flat": 1.0 / 16, "peaky": 4.0}[family])
    else:
        # ONE needle per (session, head): key 8 q against N(0, 1) keys (score 8 sqrt(Dh) >= 45), its value row of +-{1 .. 6}; a decoy is
        # the key 16 q one position outside what the named row may attend.  Every row of a session asks with the same q = +-1.
        sg = ac._signs(rng, (n, H, Dh))
        q = np.repeat(sg, F, axis=0)
        needles, decoys, named = {}, {}, {}
        for i, (p0, (base, Lr)) in enumerate(zip(shape.starts, virt)):
            first, last, ctx = p0, p0 + F - 1, shape.context
            mid = min(F - 1, 37 if F > 37 else F // 2)
            where = {"oldest_first": (max(first - ctx + 1, 0), first, max(first - ctx + 1, 0) - 1),
                     "oldest_last": (max(last - ctx + 1, 0), last, max(last - ctx + 1, 0) - 1),
                     "newest_ring": (p0 - 1, first, None), "first_staged": (p0, first, None), "last_staged": (last, last, None),
                     "own": (p0 + mid, p0 + mid, None), "future_decoy": (p0 + mid, p0 + mid, p0 + mid + 1)}[family]
            pn, prow, pd = where
            if pn < base:                      # an empty ring has no newest row: the needle falls on the first staged row instead
                pn = p0
            needles[i], named[i] = pn, prow
            if pd is not None and base <= pd <= last:
                decoys[i] = pd
            vals = ac._needle_values(rng, H, Dh)
            for h in range(H):
                Kv[i][h, pn - base] = 8.0 * sg[i, h]
                Vv[i][h, pn - base] = vals[h]
                if i in decoys:
                    Kv[i][h, decoys[i] - base] = 16.0 * sg[i, h]
        note.update(needles=needles, decoys=decoys, named=named)
    return _assemble(form, Dh, shape, q, Kv, Vv, note, never, staged_fill)


# ---- running the tap ---------------------------------------------------------------------------------------------------------------------
def run(lm, L: Launch) -> np.ndarray:
    """bf16 bits uint16 [rows, H, Dh]."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
    out = lm.debug_prefill_attn(t(L.q).to(torch.bfloat16), t(L.row_ring), t(L.row_pos), t(L.k_ring), t(L.v_ring), t(L.k_staged), t(L.v_staged),
                                cap=CAP, context=L.shape.context, ring=L.form, n_blocks=len(L.shape.starts), rings=len(L.shape.starts))
    return ac.bf16_bits(out).reshape(len(L.row_ring), H, L.Dh)


def check_tolerance(lm, form, Dh, shape, family):
    L = build(form, Dh, shape, family)
    got = bf16_bits_to_f32(run(lm, L)).astype(np.float64)
    tol = ac.tolerance(L.ref, L.A)
    with np.errstate(invalid="ignore"):
        ratio = np.where(np.isfinite(got), np.abs(got - L.ref) / tol, np.inf)
    worst = float(ratio.max())
    print(f"{family} {form} Dh={Dh} {shape.name}: worst |out - ref| / tolerance = {worst:.3f}")
    if not worst <= 1.0:
        r, h, d = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{family} {form} Dh={Dh} {shape.name}: {worst:.3g} x the tolerance at row {r} (position {int(L.row_pos[r])}) head {h} "
                             f"dim {d}: {got[r, h, d]!r} against {L.ref[r, h, d]!r}; {int((ratio > 1).sum())} elements out")


def check_needle(lm, form, Dh, shape, family):
    """Every row to which the reference gives the needle a weight of 1 - 2^-30 or more returns the needle's value row bit for bit; the row
    the needle is named after is one of them; and where a decoy exists, the named row would have found it had the mask let it."""
    L = build(form, Dh, shape, family)
    got = run(lm, L)
    F = shape.F
    for i, pn in L.note["needles"].items():
        rows = np.arange(i * F, (i + 1) * F)
        v = L.vidx[(i, pn)]
        w = L.p[rows][:, :, v]                                        # [F, H]
        sure = (w >= 1 - 2.0 ** -30).all(-1)
        named = L.note["named"][i] - shape.starts[i]
        assert sure[named], f"{family} {form} Dh={Dh} {shape.name}: the reference gives the needle only {w[named]} at its own row {named}"
        if i in L.note["decoys"]:
            vd = L.vidx[(i, L.note["decoys"][i])]
            assert not L.mask[rows[named], vd], "the decoy is not outside what the named row attends"
        want = L.Vd[rows[0]][:, v]                                    # [H, Dh]
        assert np.array_equal(ac.bf16_round(want), want)
        want_bits = (want.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
        bad = [int(r) for r in np.nonzero(sure)[0] if not np.array_equal(got[rows[r]], want_bits)]
        assert not bad, (f"{family} {form} Dh={Dh} {shape.name}: session {i}, needle at position {pn}: rows {bad[:8]} of {int(sure.sum())} "
                         f"do not return it, e.g. {bf16_bits_to_f32(got[rows[bad[0]], 0, :4])} against {want[0, :4]}")


def check_outside(lm, form, Dh, shape, pattern, j0):
    """NaN / the largest finite values in the ring's never-written slots and in the staged rows >= j0 - rows behind every query < j0,
    at any j0, inside a query tile too: rows < j0 of every block equal the run on zeros there, bit for bit, and are finite."""
    zero = run(lm, build(form, Dh, shape, "random", "zero", ("zero", j0)))
    got = run(lm, build(form, Dh, shape, "random", pattern, (pattern, j0)))
    keep = (np.arange(len(got)) % shape.F) < j0
    assert np.isfinite(bf16_bits_to_f32(got[keep])).all(), f"{pattern} outside, {form} Dh={Dh} {shape.name}: rows are not finite"
    assert np.array_equal(got[keep], zero[keep]), (f"{pattern} outside, {form} Dh={Dh} {shape.name}: differs from the zero-filled run, first at row "
                                                   f"{int(np.argwhere((got != zero).any((1, 2)) & keep)[0][0])}")


ATTN_GRID = [(form, Dh) for form in ac.FORMS for Dh in ac.HEAD_DIMS]


def check_attention(lm, form, Dh):
    for shape in SHAPES:
        for family in TOL_FAMILIES:
            check_tolerance(lm, form, Dh, shape, family)
    for shape in SHAPES[1:]:
        for family in NEEDLES:
            check_needle(lm, form, Dh, shape, family)
    # short ring / empty ring / two sessions / a window shorter than the ring; first row of a tile, inside a tile, last row of a tile
    for shape, j0 in ((SHAPES[3], 5), (SHAPES[3], 32), (SHAPES[4], 37), (SHAPES[4], 64), (SHAPES[6], 31), (SHAPES[7], 70)):
        check_outside(lm, form, Dh, shape, "nan", j0)
        check_outside(lm, form, Dh, shape, "garbage", j0)


def measure_gamma(verbose=True):
    """Worst |fp32_twin - ref| / (2^-24 A) over every tolerance launch: GAMMA = 4 x this (never measured from the kernel)."""
    worst = (0.0, None)
    for form, Dh in ATTN_GRID:
        for shape in SHAPES:
            for family in TOL_FAMILIES:
                L = build(form, Dh, shape, family)
                tw = ac.fp32_twin(L.q, L.Kd, L.Vd, L.mask).astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    r = np.maximum(np.abs(tw - L.ref) - ac.FLOOR, 0) / (2.0 ** -24 * L.A)
                r = float(np.nanmax(np.where(L.A > 0, r, 0)))
                if verbose:
                    print(f"{form} Dh={Dh} {shape.name} {family}: ratio {r:.2f}", flush=True)
                if r > worst[0]:
                    worst = (r, (form, Dh, shape.name, family))
    return worst


# ==== Part B: the call ===================================================================================================================
def frames(cfg, n, T, seed):
    """(user codes [n, n_q - dep_q, T], tokens [n, 1 + dep_q, T]) int64: what T steps would be given and would store."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, cfg.card, (n, cfg.n_q - cfg.dep_q, T))
    toks = np.concatenate([rng.integers(0, cfg.text_card, (n, 1, T)), rng.integers(0, cfg.card, (n, cfg.dep_q, T))], 1)
    return codes.astype(np.int64), toks.astype(np.int64)


def model(device, lib, cfg, rows=None, prefill_rows=None, seed=21, **kw):
    size = dict(max_rows=rows) if rows and rows > 64 else dict(max_batch=rows or 8)
    return LMModel(cached_lm_state_dict(cfg, seed), cfg, device=device, lib=lib, prefill_rows=prefill_rows, **size, **kw)


def step_forced(gen, B, sessions, codes, toks):
    """The definition's right-hand side: T forced steps under an exec mask of exactly `sessions`, the previous mask (all ones) restored."""
    dev = gen.device
    mask = torch.zeros(B, dtype=torch.bool)
    mask[list(sessions)] = True
    gen.set_exec_mask(mask.to(dev))
    n_user, nq = codes.shape[1], toks.shape[1]
    for f in range(codes.shape[2]):
        c = np.zeros((B, n_user, 1), np.int64)
        t = np.zeros((B, nq), np.int64)
        c[list(sessions), :, 0] = codes[:, :, f]
        t[list(sessions)] = toks[:, :, f]
        gen._step(torch.from_numpy(c).to(dev), False, None, torch.from_numpy(t).to(dev))
    gen.set_exec_mask(torch.ones(B, dtype=torch.bool).to(dev))


def state_of(gen):
    """{region: uint8 [rows or 1, bytes per row]} of the kind-1 regions (what a session is), rng cut to its first word."""
    buf = gen.get_streaming_state()["lm_gen"].cpu().numpy()
    out = {}
    for name, (off, nbytes, rows, kind) in gen.state_regions().items():
        if kind != 1:
            continue
        if name == "rng":
            nbytes = 8                                              # rng[1], the draw counter, is the one word that may differ
        out[name] = buf[off:off + nbytes].reshape(max(rows, 1), -1).copy()
    return out


def deeper_ring(name):
    return name[:3] in ("kc.", "vc.") and not name.split(".")[1] == "0"


def compare_states(a, b, sessions, what, rings="layer0"):
    """Regions of state `a` and `b` equal for `sessions` (None = all rows); rings: "layer0" leaves the rings of layers >= 1 out, "none"
    every ring, "all" none."""
    assert sorted(a) == sorted(b)
    for name in a:
        ring = name[:3] in ("kc.", "vc.")
        if (ring and rings == "none") or (deeper_ring(name) and rings == "layer0"):
            continue
        x, y = a[name], b[name]
        if sessions is not None and x.shape[0] > 1:
            x, y = x[list(sessions)], y[list(sessions)]
        assert np.array_equal(x, y), f"{what}: region {name} differs ({int((x != y).any(-1).sum())} of {x.shape[0]} rows)"


def check_rings_and_state(device, lib, kv="bf16", starts=(0,), T=40, B=65, prefill_rows=128, seed=5, active=None, stats=None):
    """Cases 2 and 3: sessions `range(len(starts))` of a B-session stream, moved to `starts`, take T frames by prefill on one handle and
    by forced steps on its twin.  Layer-0 rings and every other state region of the named sessions are identical; the regions of the
    sessions not named equal their state before the call (all rings included)."""
    cfg = replace(tiny_lm_config(), kv_cache_dtype=kv) if kv != "bf16" else tiny_lm_config()
    n = len(starts)
    sess = list(range(n))
    codes, toks = frames(cfg, n, T, seed)
    offs = list(starts) + [0] * (B - n)
    res = {}
    for how in ("prefill", "steps"):
        gen = LMGen(model(device, lib, cfg, rows=B, prefill_rows=prefill_rows if how == "prefill" else None), use_sampling=False,
                    support_out_of_sync=True)
        with gen.streaming(B):
            gen.seek(offs)
            if active is not None:
                m = [b == active for b in range(B)]
                gen.set_session_sampling([SessionSampling(repetition_penalty=1.3, repetition_context=32, seed=3)] * B, mask=m)
            before = state_of(gen)
            if how == "prefill":
                gen.prefill(torch.from_numpy(codes), torch.from_numpy(toks), sessions=sess)
            else:
                step_forced(gen, B, sess, codes, toks)
            res[how] = (before, state_of(gen), int(gen._lib.mmi_lm_stat(gen.lm_model._handle, 4)))
    (b0, a0, rl0), (_, a1, rl1) = res["prefill"], res["steps"]
    if stats is not None:
        stats.update(rows_launches=(rl0, rl1))
    others = [b for b in range(B) if b not in sess]
    compare_states(b0, a0, others, f"{kv} ring: sessions not named, against their state before the prefill", rings="all")
    compare_states(a0, a1, sess, f"{kv} ring, starts {starts}, T={T}: prefill against forced steps")
    assert int(a0["offsets"].view(np.int64)[0, 0]) == starts[0] + T
    if active is not None:
        assert int(a0["rowtab"][active].view(np.uint32).max()) > 0 and a0["thist"][active].any(), "the text history was not exercised"


def check_network_vs_oracle(device, lib, kind="moshi", T=12, prefill_rows=128, kv="bf16", cond=False, B=2, seed=901):
    """Case 4: the oracle steps T greedy frames; its codes and stored tokens are prefilled into the engine; both then step
    max_delay + 3 further frames with the oracle's tokens forced (lm_cases.oracle_vs_engine's loop and gates, unchanged)."""
    cfg = tiny_lm_config() if kind == "moshi" else tiny_stt_config()
    if kv != "bf16":
        cfg = replace(cfg, kv_cache_dtype=kv)
    sd = cached_lm_state_dict(cfg, seed)
    kw, okw = {}, {}
    if cond:
        from moshi_amd.lm import ConditionFuser
        rng = np.random.default_rng(seed)
        cs = torch.from_numpy(0.5 * rng.standard_normal((B, 1, cfg.dim)).astype(np.float32)).to(torch.bfloat16)
        kw = dict(fuser=ConditionFuser({"sum": ["c"]}))
        okw = dict(condition_tensors={"c": (cs, None)})
    lm = LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=prefill_rows, **kw)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, **okw)
    orc = LMOracle(sd, cfg)
    if kv == "fp4":
        from tests.kv4_cases import Kv4Oracle
        orc = Kv4Oracle(sd, cfg)
    if cond:
        orc.streaming(B, condition_sum=cs.float().numpy().reshape(B, cfg.dim))
    else:
        orc.streaming(B)
    rng = np.random.default_rng(seed + 1)
    n_user = cfg.n_q - cfg.dep_q
    codes = rng.integers(0, cfg.card, (B, n_user, T)).astype(np.int64)
    toks = np.zeros((B, 1 + cfg.dep_q, T), np.int64)
    for f in range(T):
        _, (_, _, ott, oat) = orc.step(codes[:, :, f:f + 1], use_sampling=False, support_out_of_sync=True)
        toks[:, 0, f], toks[:, 1:, f] = ott, oat
    with gen.streaming(B):
        gen.prefill(torch.from_numpy(codes), torch.from_numpy(toks))
        for s in range(max(cfg.delays) + 3):
            c = rng.integers(0, cfg.card, (B, n_user, 1))
            oo, (otl, oal, ott, oat) = orc.step(c, use_sampling=False, support_out_of_sync=True)
            forced = np.concatenate([ott[:, None], oat], 1)
            out, tl, al = gen.step_with_taps(torch.from_numpy(c).to(device), forced_tokens=torch.from_numpy(forced).to(device))
            assert out is not None or T + s < max(cfg.delays) + 1
            if out is not None:
                assert np.array_equal(out.cpu().numpy(), oo), f"T={T} step {s}: ring output differs (the delay ring's tail)"
            tl, al = tl.cpu().numpy(), al.cpu().numpy()
            for b in range(B):
                assert lc.logits_close(tl[b], otl[b]), f"T={T} step {s} row {b}: text logits {np.abs(tl[b] - otl[b]).max()}"
                t_e, t_o = int(tl[b].argmax()), int(ott[b])
                assert t_e == t_o or lc.near_tie(otl[b], t_e, t_o)
                for k in range(cfg.dep_q):
                    assert lc.logits_close(al[b, k], oal[b, k]), f"T={T} step {s} row {b} cb {k}: {np.abs(al[b, k] - oal[b, k]).max()}"
                    a_e, a_o = int(al[b, k].argmax()), int(oat[b, k])
                    assert a_e == a_o or lc.near_tie(oal[b, k], a_e, a_o)


def check_between_steps_of_a_live_batch(device, lib, B=8, picked=(2, 5), T=20):
    """Case 5: eight sessions stream with sampling; after step 3 sessions 2 and 5 are reset and prefilled with 20 frames.  The other
    six sessions' tokens over the next 6 steps are those of a run in which 2 and 5 were merely reset and left idle (exec mask off);
    2 and 5 then produce valid frames."""
    cfg = tiny_lm_config()
    rng = np.random.default_rng(17)
    n_user = cfg.n_q - cfg.dep_q
    live = [torch.from_numpy(rng.integers(0, cfg.card, (B, n_user, 1))).to(device) for _ in range(9)]
    codes, toks = frames(cfg, len(picked), T, 23)
    outs = {}
    for how in ("prefill", "idle"):
        gen = LMGen(model(device, lib, cfg, rows=B, prefill_rows=16), use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=5,
                    support_out_of_sync=True)
        got = []
        with gen.streaming(B):
            for c in live[:3]:
                gen.step(c)
            m = torch.zeros(B, dtype=torch.bool)
            m[list(picked)] = True
            gen.reset_streaming(m.to(device))
            if how == "prefill":
                gen.prefill(torch.from_numpy(codes), torch.from_numpy(toks), sessions=picked)
            else:
                gen.set_exec_mask((~m).to(device))
            for c in live[3:]:
                got.append(gen.step(c)[:, :, 0].cpu().numpy())
        outs[how] = got
    others = [b for b in range(B) if b not in picked]
    for s, (a, b) in enumerate(zip(outs["prefill"], outs["idle"])):
        assert np.array_equal(a[others], b[others]), f"step {s} after the prefill: a neighbour's tokens depend on it"
    last = outs["prefill"][-1][list(picked)]
    assert (last >= 0).all() and (last[:, 0] < cfg.text_card).all() and (last[:, 1:] < cfg.card).all(), last
    assert any((o[others] >= 0).all() for o in outs["prefill"]), "no step produced tokens: nothing shown"


def check_chunking(device, lib, budgets=(128, 32, 5), T=23, starts=(0, 9), B=3):
    """Case 6: the same call at other row budgets: identical non-ring state; the next steps' logits agree under the gates of case 4.
    Layer-0 rings are identical between budgets whose passes take the same GEMM kernels (here: all of them, k_gemm_xp at <= 64 rows)."""
    cfg = tiny_lm_config()
    n = len(starts)
    codes, toks = frames(cfg, n, T, 31)
    rng = np.random.default_rng(4)
    nxt = [torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device) for _ in range(3)]
    res = []
    for rows in budgets:
        gen = LMGen(model(device, lib, cfg, rows=32, prefill_rows=rows), use_sampling=False, support_out_of_sync=True)
        with gen.streaming(B):
            gen.seek(list(starts) + [0] * (B - n))
            gen.prefill(torch.from_numpy(codes), torch.from_numpy(toks), sessions=range(n))
            st = state_of(gen)
            lg = [tuple(t.cpu().numpy() for t in gen.step_with_taps(c)[1:]) for c in nxt]
        res.append((st, lg))
    ref = res[0][1]
    for (st, lg), rows in zip(res[1:], budgets[1:]):
        compare_states(res[0][0], st, range(n), f"prefill_rows {budgets[0]} against {rows}")
        for s in range(len(nxt)):
            for b in range(n):
                what = f"prefill_rows {rows}: step {s} row {b}"
                assert lc.logits_close(lg[s][0][b], ref[s][0][b]), f"{what}: text logits"
                t_a, t_b = int(lg[s][0][b].argmax()), int(ref[s][0][b].argmax())
                assert t_a == t_b or lc.near_tie(ref[s][0][b], t_a, t_b), f"{what}: greedy text tokens part away from a tie"
                for k in range(cfg.dep_q):
                    assert lc.logits_close(lg[s][1][b, k], ref[s][1][b, k]), f"{what} cb {k}: audio logits"
                    a_a, a_b = int(lg[s][1][b, k].argmax()), int(ref[s][1][b, k].argmax())
                    assert a_a == a_b or lc.near_tie(ref[s][1][b, k], a_a, a_b), f"{what} cb {k}: greedy audio tokens part away from a tie"


def check_last_tokens_log(device, lib, B=2, steps=15):
    """Case 8: a log built from last_tokens() over 15 sampled steps, prefilled into a fresh session, reproduces the original sessions'
    non-ring state and layer-0 rings."""
    cfg = tiny_lm_config()
    rng = np.random.default_rng(40)
    codes = rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, steps)).astype(np.int64)
    mine = SessionSampling(temp=0.7, temp_text=0.9, top_k=12, top_k_text=7, seed=11, repetition_penalty=1.2, repetition_context=16)
    gen = LMGen(model(device, lib, cfg, rows=B, prefill_rows=16), use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=5,
                support_out_of_sync=True)
    log = []
    with gen.streaming(B):
        gen.set_session_sampling(mine)
        for f in range(steps):
            gen.step(torch.from_numpy(codes[:, :, f:f + 1]).to(device))
            log.append(gen.last_tokens().cpu().numpy())
        want = state_of(gen)
    toks = np.stack(log, -1)
    assert toks.shape == (B, 1 + cfg.dep_q, steps) and (toks >= 0).all()
    with gen.streaming(B):
        gen.set_session_sampling(mine)
        gen.prefill(torch.from_numpy(codes), torch.from_numpy(toks))
        got = state_of(gen)
    compare_states(want, got, None, "a session rebuilt from its last_tokens() log")


def check_refusals_and_off_state(device, lib):
    """Case 7."""
    import pytest
    from moshi_amd.lm import ConditionFuser
    from moshi_amd.weights import quantize_lm_state_dict, quantize_lm_state_dict_fp8, quantize_lm_state_dict_mxfp4
    cfg = tiny_lm_config()
    sd = cached_lm_state_dict(cfg, 21)
    with pytest.raises(NotImplementedError, match="at most 128 rows"):
        LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=129)
    with pytest.raises(NotImplementedError, match="16-row tile"):
        LMModel(sd, cfg, device=device, lib=lib, max_batch=16, prefill_rows=33)
    LMModel(sd, cfg, device=device, lib=lib, max_batch=16, prefill_rows=32)
    for q in (quantize_lm_state_dict, quantize_lm_state_dict_fp8):
        with pytest.raises(NotImplementedError, match="quantised linears"):
            LMModel(q(sd), cfg, device=device, lib=lib, max_batch=32, prefill_rows=32)
    from tests.mxfp4_cases import mx_config
    with pytest.raises(NotImplementedError, match="quantised linears"):
        LMModel(quantize_lm_state_dict_mxfp4(cached_lm_state_dict(mx_config(), 21)), mx_config(), device=device, lib=lib, max_batch=32, prefill_rows=32)
    with pytest.raises(NotImplementedError, match="adapter handles"):
        LMModel(sd, cfg, device=device, lib=lib, max_batch=32, adapters=(2, 32), prefill_rows=32)
    from tests import row_condition_cases as rcc
    xcfg = rcc.tiny_cross_config()
    with pytest.raises(NotImplementedError, match="cross-attention"):
        LMModel(cached_lm_state_dict(xcfg, 21), xcfg, device=device, lib=lib, max_batch=32, prefill_rows=32, fuser=ConditionFuser({"cross": ["x"]}))
    n_user = cfg.n_q - cfg.dep_q
    codes, toks = frames(cfg, 2, 3, 1)
    tc, tt = torch.from_numpy(codes), torch.from_numpy(toks)
    lm = LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=4)
    assert lm._lib.mmi_lm_prefill_rows(lm._handle) == 4
    # the TTS machine, hooks and guidance arrive with the stream
    from moshi_amd.lm import TTSMachine
    with pytest.raises(NotImplementedError, match="TTS machine"):
        LMGen(lm, use_sampling=False, tts_machine=TTSMachine(text_card=cfg.text_card + 1)).streaming_forever(2)
    lm._lib.check(lm._lib.mmi_lm_streaming_stop(lm._handle))
    gen = LMGen(lm, use_sampling=False, on_text_hook=lambda t: None)
    with gen.streaming(2):
        with pytest.raises(NotImplementedError, match="hooks"):
            gen.prefill(tc, tt)
    cs = torch.zeros(4, 1, cfg.dim, dtype=torch.bfloat16)
    glm = LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=4, fuser=ConditionFuser({"sum": ["c"]}))
    gen = LMGen(glm, use_sampling=False, cfg_coef=2.0, condition_tensors={"c": (cs, None)})
    with gen.streaming(2):
        with pytest.raises(NotImplementedError, match="guided"):
            gen.prefill(tc, tt)
    gen = LMGen(lm, use_sampling=False)
    with pytest.raises(RuntimeError, match="streaming"):
        gen.prefill(tc, tt)
    with gen.streaming(3):
        with pytest.raises(RuntimeError, match="not while streaming"):
            lm._lib.check(lm._lib.mmi_lm_enable_prefill(lm._handle, 8))
        with pytest.raises(ValueError, match="out of range"):
            gen.prefill(tc, tt, sessions=[0, 3])
        with pytest.raises(ValueError, match="named twice"):
            gen.prefill(tc, tt, sessions=[1, 1])
        with pytest.raises(ValueError, match="T must be"):
            import ctypes as C
            dc, dt = tc.to(device), tt.to(device)
            lm._lib.check(lm._lib.mmi_lm_prefill(lm._handle, (C.c_int32 * 2)(0, 1), 2, dc.data_ptr(), dt.data_ptr(), 0, None))
        with pytest.raises(ValueError, match="sessions per call"):
            gen.prefill(torch.zeros(5, n_user, 1, dtype=torch.int64), torch.zeros(5, 1 + cfg.dep_q, 1, dtype=torch.int64), sessions=[0, 1, 2, 0, 1])
        before = state_of(gen)
        with pytest.raises(AssertionError, match="forced"):
            LMGen.prefill(_checked(gen), tc, -tt - 1, sessions=[0, 1])
        compare_states(before, state_of(gen), None, "a refused call", rings="all")
    # the off state: a handle without prefill_rows is what it was, with and without an enabled handle next to it
    rng = np.random.default_rng(2)
    steps = [torch.from_numpy(rng.integers(0, cfg.card, (2, n_user, 1))).to(device) for _ in range(3)]

    def off_run():
        plain = LMModel(sd, cfg, device=device, lib=lib, max_batch=32)
        assert plain._lib.mmi_lm_prefill_rows(plain._handle) == 0
        g = LMGen(plain, use_sampling=True, seed=9, support_out_of_sync=True)
        with g.streaming(2):
            toks_ = [g.step(c)[:, :, 0].cpu().numpy() for c in steps]
            snap = (state_of(g), int(g.get_streaming_state()["lm_gen"].numel()))      # (scratch a stream never wrote is not compared)
            with pytest.raises(RuntimeError, match="prefill is not enabled"):
                g.prefill(tc, tt)
            return [f"{a}\t{b}" for a, b in g.launch_list()], int(g._lib.mmi_lm_state_bytes(plain._handle)), snap, toks_
    a = off_run()
    on = LMGen(LMModel(sd, cfg, device=device, lib=lib, max_batch=32, prefill_rows=32), use_sampling=True, seed=9, support_out_of_sync=True)
    with on.streaming(2):
        on_toks = [on.step(c)[:, :, 0].cpu().numpy() for c in steps]
        on_bytes, on_list = int(on._lib.mmi_lm_state_bytes(on.lm_model._handle)), [f"{x}\t{y}" for x, y in on.launch_list()]
        b = off_run()
    assert a[0] == b[0] == on_list, "the launch list of a step changed"
    assert a[1] == b[1] == on_bytes == a[2][1] == b[2][1], "mmi_lm_state_bytes / the snapshot's size changed"
    compare_states(a[2][0], b[2][0], None, "a handle without prefill_rows, alone and next to an enabled handle", rings="all")
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a[3], b[3], on_toks))
    assert not any("k_pf_" in k or "prefill" in k for k in a[0])


def _checked(gen):
    gen.check = True
    return gen


def wide_layer_config(kv="bf16"):
    """One temporal layer at the production width (dim 4096, 32 heads of 128, FFN 11264: mxfp4_cases.check_7b_layer_shapes' recipe) with a
    context of 64; small vocabularies keep the embedding tables out of the way."""
    cfg = replace(tiny_lm_config(), card=72, dim=4096, num_heads=32, num_layers=1, hidden_scale=4.125, context=64, text_card=64)
    assert cfg.ffn_hidden == 11264
    return replace(cfg, kv_cache_dtype=kv) if kv != "bf16" else cfg


def check_production_width(device, lib, kv, n, T, B=65, seed=77):
    """Case 9 (GPU): n sessions x T frames = 128 rows in one pass at the production width against a twin that steps the same frames at 65
    rows (both in_proj through k_gemm_rows): layer-0 rings bit-identical, the non-ring state identical, and the following step's
    logits under the gates.  T = 128 > context: the pass wraps the ring twice."""
    cfg = wide_layer_config(kv)
    sess = list(range(n))
    codes, toks = frames(cfg, n, T, seed)
    rng = np.random.default_rng(seed)
    nxt = torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device)
    res = {}
    for how in ("prefill", "steps"):
        gen = LMGen(model(device, lib, cfg, rows=128, prefill_rows=128 if how == "prefill" else None, seed=seed), use_sampling=False,
                    support_out_of_sync=True)
        with gen.streaming(B):
            if how == "prefill":
                gen.prefill(torch.from_numpy(codes), torch.from_numpy(toks), sessions=sess)
            else:
                step_forced(gen, B, sess, codes, toks)
            st = state_of(gen)
            rl = int(gen._lib.mmi_lm_stat(gen.lm_model._handle, 4))
            _, tl, al = gen.step_with_taps(nxt)
            res[how] = (st, tl.cpu().numpy(), al.cpu().numpy(), rl)
    a, b = res["prefill"], res["steps"]
    assert a[3] > 0 and b[3] > 0, "a side did not run k_gemm_rows"
    compare_states(a[0], b[0], sess, f"production width, {kv} ring, {n} x {T} rows: prefill against forced steps", rings="all")
    for s in sess:
        assert lc.logits_close(a[1][s], b[1][s]), f"session {s}: text logits of the following step"
        for k in range(cfg.dep_q):
            assert lc.logits_close(a[2][s, k], b[2][s, k]), f"session {s} cb {k}: audio logits of the following step"
