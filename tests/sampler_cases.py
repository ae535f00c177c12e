"""The sampler (lm_kernels.h k_sample) token for token on crafted logit rows, shared by the simulator and the GPU tests.

`LMGen(on_text_logits_hook=...)` overwrites the bf16 text logits just before k_sample runs at site 0 and `on_text_hook` sees the
token it picked, so a tiny LM whose `text_card` is V drives the instantiation add_sample chooses for V (<256,8>, <1024,8>,
<1024,32>) with any row.  Every row family below aims at one branch of the kernel: the window of 8 high bytes under the block
maximum and the two-pass fallback below it, the plateau at the threshold (the `cnt_at_t == want_eq` shortcut against the scanned
split), the per-vector skip, the packed per-thread counters, -inf members of the set, and the two ends of the uniform draw.

The reference is numpy in float64: stable sort on (-value, index), first k; u and the score as the kernel documents them; argmax.
It shares the Philox restatement (lm_cases.philox4_words / philox_exp_noise) with the older tests and nothing with the kernel's
select.  A row is used only where the reference's two best scores differ by more than MARGIN * max(1, |best|) - 50 x the 2e-5
that lm_cases.check_topk_device_rng grants the device's logarithm - and on every used row the engine's token must EQUAL the
reference's; a row that fails the condition is regenerated from the next seed, and at most 2 % may be.

Left out on purpose: +-0 as a threshold value and NaN logits - the order torch.topk gives equal or unordered floats is
unspecified in the reference, so there is nothing to hold the kernel to.  The window family needs k >= 2 (with k = 1 the k-th
largest key IS the maximum) and the f < k sparse rows need k >= 2 as well.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config
from moshi_amd.lm import LMGen, LMModel
from tests.lm_cases import cached_lm_state_dict, philox4_words, philox_exp_noise

VOCABS = (1000, 2048, 8192, 32000)
KS = (1, 10, 25, 250, 255, 256)
MARGIN = 1e-3
B = 8
TEMP = {1: 1.0, 10: 0.7, 25: 0.8, 250: 1.0, 255: 0.7, 256: 0.9, 0: 0.8}      # per engine (k = 0: the full multinomial)
AUDIO_TOP_K = 20
dropped = {"rows": 0, "regenerated": 0}


def geometry(V: int):
    """(threads, entries per thread) of the k_sample instantiation add_sample picks for V (lm_engine.hip)."""
    return (256, 8) if V <= 2048 else (1024, 8) if V <= 8192 else (1024, 32)


def bf16(x) -> np.ndarray:
    """Round to bf16 (nearest even), back as float32; +0.0 is added so that no -0 survives."""
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy() + np.float32(0.0)


def from_keys(key: np.ndarray) -> np.ndarray:
    """Order-preserving 16-bit key (sign bit set: the bf16 bits of a positive value; clear: the complement of a negative's)
    -> float32."""
    key = np.asarray(key, np.int64)
    bits = np.where(key & 0x8000, key & 0x7FFF, (~key) & 0xFFFF).astype(np.uint32)
    return (bits << np.uint32(16)).view(np.float32)


# ---- the draws -------------------------------------------------------------------------------------------------------------------
def _uniform(words: np.ndarray) -> np.ndarray:
    """u as the kernel documents it: the word's top 24 bits + 0.5, in fp32 (above 2^23 the sum is rounded to even), times 2^-24,
    clamped to the largest float under 1 - which only the all-ones word reaches.  Strictly inside (0, 1); returned as float64."""
    n = (words >> np.uint64(8)).astype(np.float32)
    u = np.minimum((n + np.float32(0.5)) * np.float32(2.0 ** -24), np.float32(1.0 - 2.0 ** -24))
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
    return u.astype(np.float64)


def uniform_fast(seed: int, step: int, a: int, idx: np.ndarray) -> np.ndarray:
    """u of entry idx on the fast path: word (i & 3) of Philox4x32-10 at counter (step, a, i >> 2)."""
    idx = np.asarray(idx, np.int64)
    return _uniform(philox4_words(seed, step, a, idx >> 2)[np.arange(len(idx)), idx & 3])


def uniform_entry(seed: int, step: int, a: int, idx: np.ndarray) -> np.ndarray:
    """u of mmi_exp_noise (the full multinomial): word 0 at counter (step, a, i)."""
    return _uniform(philox4_words(seed, step, a, np.asarray(idx, np.int64))[:, 0])


# ---- the float64 references --------------------------------------------------------------------------------------------------------
def topk_set(x: np.ndarray, k: int) -> np.ndarray:
    xd = x.astype(np.float64)
    return np.lexsort((np.arange(len(xd)), -xd))[:min(k, len(xd))]          # (-value, index), first k: rank order


def _winner(members: np.ndarray, score: np.ndarray):
    """(token, decided): the member with the largest score; decided = the runner-up is further than the tie rule asks."""
    o = np.argsort(-score, kind="stable")
    best = score[o[0]]
    second = score[o[1]] if len(o) > 1 else -np.inf
    return int(members[o[0]]), bool(best - second > MARGIN * max(1.0, abs(best)))


def ref_fast(x, k, temp, seed, step, a):
    """(a) top-k, device RNG: x / temp - ln(-ln u) over the set."""
    m = topk_set(x, k)
    with np.errstate(divide="ignore"):
        return _winner(m, x[m].astype(np.float64) / temp - np.log(-np.log(uniform_fast(seed, step, a, m))))


def ref_ranked(x, k, temp, noise):
    """(b) supplied noise: the draw of a member is indexed by its rank in the set."""
    m = topk_set(x, k)
    return _winner(m, x[m].astype(np.float64) / temp - np.log(noise[:len(m)].astype(np.float64)))


def ref_full(x, temp, seed, step, a):
    """(c) top_k = 0: every entry competes with its own draw."""
    idx = np.arange(len(x))
    with np.errstate(divide="ignore"):
        return _winner(idx, x.astype(np.float64) / temp - np.log(-np.log(uniform_entry(seed, step, a, idx))))


def oracle_full(x, temp, seed, step, a):
    """The rule lm_cases.check_full_multinomial holds the engine to: fp32 softmax over the draws of philox_exp_noise."""
    z = (x / np.float32(temp)).astype(np.float32)
    pr = np.exp(z - z.max()).astype(np.float32)
    pr = pr / pr.sum(dtype=np.float32)
    return int(np.argmax(pr / philox_exp_noise(seed, step, a, np.arange(len(x)))))


def oracle_ranked_is_unambiguous(x, k, temp) -> bool:
    """oracle.lm_oracle.sample_token ranks by the fp32 PROBABILITY, the kernel by the logit: the two orders part where distinct
    logits share a probability.  That is harmless where the shared probability is 0 (such a member scores 0 and cannot win)."""
    z = (x / np.float32(temp)).astype(np.float32)
    e = np.exp(z - z.max()).astype(np.float32)
    p = (e / e.sum(dtype=np.float32)).astype(np.float32)
    op = np.lexsort((np.arange(len(x)), -p))[:k]
    ox = topk_set(x, k)
    diff = op != ox
    return bool(np.all(p[op[diff]] == 0) and np.all(p[ox[diff]] == 0))


# ---- row families --------------------------------------------------------------------------------------------------------------------
def _edges(V, rng):
    """Indices where an off-by-one in the kernel's index arithmetic would show: both ends, both sides of thread, vector and wave
    boundaries (thread t owns [t * E, t * E + E), a vector is 8 entries, a wave 64 threads)."""
    NT, E = geometry(V)
    out = {0, 1, V - 1, V - 2, 7, 8, 15, 16}
    for t in rng.integers(1, (V + E - 1) // E, 6):
        out |= {int(t) * E - 1, int(t) * E}
    for w in range(1, NT // 64):
        if w * 64 * E < V:
            out |= {w * 64 * E - 1, w * 64 * E}
    for v in rng.integers(1, V // 8, 4):
        out |= {int(v) * 8 - 1, int(v) * 8}
    return np.array(sorted(i for i in out if 0 <= i < V))


def _scatter(V, n, rng, must=()):
    """n distinct indices: the edge indices first (a random subset if there are more than n), random ones after."""
    must = [i for i in must if 0 <= i < V]
    e = [i for i in _edges(V, rng) if i not in must]
    rng.shuffle(e)
    pick = (list(must) + e)[:n]
    if len(pick) < n:
        rest = np.setdiff1d(np.arange(V), pick)
        pick += list(rng.choice(rest, n - len(pick), replace=False))
    return np.array(sorted(pick))


def all_equal(V, k, rng, ctx):
    return np.full(V, bf16(rng.choice([-3.25, -0.5, 0.75, 2.0, 17.0])), np.float32)


def _plateau(V, k, rng, extra, big=False):
    """m < k entries above T, n = k - m + extra entries equal to T, the rest below."""
    m = int(rng.integers(0, k)) if k > 1 else 0
    n = min(k - m + extra, V - m - 4)
    T = float(bf16(rng.choice([-2.25, -0.375, 0.625, 1.5, 3.0])))
    x = bf16(T - 0.25 - 2.0 * rng.random(V))
    at = _scatter(V, n, rng)
    x[at] = T
    rest = np.setdiff1d(np.arange(V), at)
    up = rng.choice(rest, m, replace=False)
    x[up] = bf16(T + (0.03125 if not big else 0.5) + 0.25 * rng.random(m))      # a small head start: the plateau often wins
    assert (x[up] > T).all() and (np.delete(x, np.concatenate([at, up])) < T).all()
    return x


def plateau_exact(V, k, rng, ctx):          # n == k - m: every entry at the threshold is in the set (the shortcut)
    return _plateau(V, k, rng, 0)


def plateau_plus_one(V, k, rng, ctx):       # n == k - m + 1: one entry at the threshold is left out (the scan)
    return _plateau(V, k, rng, 1)


def plateau_wide(V, k, rng, ctx):
    return _plateau(V, k, rng, int(rng.integers(2, 400)))


def plateau_on_the_draws(V, k, rng, ctx):
    """A plateau laid out on this slot's draws: the LAST plateau entry inside the set and the FIRST one outside it sit on the two
    luckiest draws of the row, so taking one entry more, one fewer or the other end of the plateau changes the winner."""
    g = ctx["gumbel"]
    if g is None:
        return _plateau(V, k, rng, 3)
    m = int(rng.integers(0, max(1, k // 4))) if k > 1 else 0
    lucky = np.argsort(-g)[:2]
    lo, hi = int(lucky.min()), int(lucky.max())
    inside = k - m                                     # plateau entries in the set: inside - 1 of them below index lo
    if lo < inside - 1 or V - hi - 1 < 3:
        return _plateau(V, k, rng, 3)
    T = 1.0
    x = bf16(T - 0.5 - 2.0 * rng.random(V))
    x[rng.choice(lo, inside - 1, replace=False) if inside > 1 else []] = T
    x[[lo, hi]] = T
    x[rng.choice(np.arange(hi + 1, V), min(3, V - hi - 1), replace=False)] = T
    free = np.nonzero(x < T)[0]
    x[rng.choice(free, m, replace=False)] = bf16(T + 0.0625)
    return x


def coarse_grid(V, k, rng, ctx):
    return bf16(0.5 * rng.integers(-4, 5, V))


def _window(V, k, rng, hmax, d, spread=12):
    """The k-th largest key exactly d high bytes under the maximum's: m < k keys in the bytes above, more than k - m in byte
    hmax - d, the rest below.  d = 7 is the last byte of the kernel's window, d = 8 the first the fallback select handles."""
    assert k >= 2
    m = int(rng.integers(1, k))
    n = min(k - m + int(rng.integers(0, 40)), V - m - 4)
    hk = hmax - d
    lo_byte = max(hk - spread, 1)
    key = (rng.integers(lo_byte, hk, V) << 8) | rng.integers(0, 256, V)
    at = _scatter(V, n, rng)
    key[at] = (hk << 8) | rng.integers(0, 256 if n > 3 else 4, n)          # few entries: a narrow range, so that some tie
    rest = np.setdiff1d(np.arange(V), at)
    up = rng.choice(rest, m, replace=False)
    key[up] = (rng.integers(hk + 1, hmax + 1, m) << 8) | rng.integers(0, 256, m)
    key[up[0]] = (hmax << 8) | int(rng.integers(0, 256))
    key = np.where((key == 0x8000) | (key == 0x7FFF), key + 2, key)           # no +-0
    x = from_keys(key)
    assert np.isfinite(x).all()
    return x


# high byte of the key: 0x80 | (sign + 7 exponent bits) for a positive value, the complement for a negative one.  The small
# magnitudes (2^-95, 2^-120) leave the decision to the draws alone, so ANY wrong member of the set can show as a wrong token.
def window_last_byte(V, k, rng, ctx):
    return _window(V, k, rng, 0x90, 7)


def window_below(V, k, rng, ctx):
    return _window(V, k, rng, 0x90, 8)


def window_cross_sign_last_byte(V, k, rng, ctx):      # positive maximum, negative k-th largest, inside the window
    return _window(V, k, rng, 0x83, 7)


def window_cross_sign_below(V, k, rng, ctx):
    return _window(V, k, rng, 0x83, 8)


def window_all_negative(V, k, rng, ctx):
    return _window(V, k, rng, 0x7D, int(rng.choice([7, 8])))


def window_unit_scale(V, k, rng, ctx):                # the same around 1.0 (bytes 0xBF .. 0xB7): here the large logits decide
    return _window(V, k, rng, 0xBF, int(rng.choice([7, 8])), spread=3)


def cross_sign_plain(V, k, rng, ctx):
    """Positive maximum, negative k-th largest at ordinary magnitudes: far below the window, the fallback select."""
    x = bf16(-0.5 - 1.5 * rng.random(V))
    up = rng.choice(V, max(1, k // 2), replace=False)
    x[up] = bf16(0.25 + 1.5 * rng.random(len(up)))
    return x


def dense_threads(V, k, rng, ctx):
    """All E entries of several threads in the maximum's high byte (0x3F..: 0.5 <= x < 2): the 8-bit per-thread counters reach E."""
    NT, E = geometry(V)
    x = bf16(0.05 + 0.2 * rng.random(V))
    for t in rng.choice((V + E - 1) // E - 1, int(rng.integers(2, 6)), replace=False):
        x[t * E:(t + 1) * E] = bf16(0.5 + 1.49 * rng.random(E))
    return x


def sparse_fewer_than_k(V, k, rng, ctx):
    f = int(rng.integers(1, k)) if k > 1 else 1
    x = np.full(V, -np.inf, np.float32)
    x[_scatter(V, f, rng)] = bf16(2.0 * rng.standard_normal(f))
    return x


def sparse_one(V, k, rng, ctx):
    x = np.full(V, -np.inf, np.float32)
    x[int(rng.choice(_edges(V, rng)))] = bf16(rng.standard_normal())
    return x


def sparse_huge(V, k, rng, ctx):
    """One entry near the largest bf16.  Fast path: 2.5e38, which / 0.7 overflows to a score of +inf there and must win all the
    same.  The softmax paths, like the reference's softmax, are undefined (inf - inf) once logit / temp overflows: they get the
    largest magnitude that stays finite after the division."""
    x = np.full(V, -np.inf, np.float32)
    at = _scatter(V, min(k + 3, 40), rng)
    x[at] = bf16(3.0 * rng.standard_normal(len(at)))
    x[int(rng.choice(at))] = bf16(2.5e38 if ctx["mode"] in "ad" else 2.5e38 * min(1.0, ctx["temp"]))
    return x


def peaked(V, k, rng, ctx):
    x = bf16(2.0 * rng.standard_normal(V))
    x[int(rng.integers(0, V))] = bf16(x.max() + 30.0)
    return x


def bland(V, k, rng, ctx):
    return bf16(3.0 * rng.standard_normal(V))


FAMILIES = [all_equal, plateau_exact, plateau_plus_one, plateau_wide, plateau_on_the_draws, plateau_on_the_draws, coarse_grid,
            coarse_grid, window_last_byte, window_below, window_cross_sign_last_byte, window_cross_sign_below, window_all_negative,
            window_unit_scale, cross_sign_plain, dense_threads, dense_threads, sparse_fewer_than_k, sparse_one, sparse_huge, peaked,
            bland, plateau_exact, plateau_plus_one]
NEEDS_K2 = {window_last_byte, window_below, window_cross_sign_last_byte, window_cross_sign_below, window_all_negative,
            window_unit_scale}


def families_for(k: int, mode: str):
    fams = [f for f in FAMILIES if k >= 2 or f not in NEEDS_K2 or mode in "cd"]
    while len(fams) % B:
        fams.append(FAMILIES[len(fams) % 7 + 1])
    return fams


# ---- the harness ---------------------------------------------------------------------------------------------------------------------
_LM = {}


def _model(device, lib, V):
    """One tiny LM per vocabulary (only `text_card` differs from tiny_lm_config()); the LMGen of every (k, mode) shares it."""
    key = (str(device), id(lib), V)
    if key not in _LM:
        _LM.clear()
        cfg = replace(tiny_lm_config(), text_card=V)
        _LM[key] = (cfg, LMModel(cached_lm_state_dict(cfg, 21), cfg, device=device, max_batch=B, lib=lib))
    return _LM[key]


def run_engine(device, lib, V, k, mode, batches, seed, noise=None, temp=None, record_logits=False):
    """One engine, one stream, len(batches) steps; step s samples site 0 from batches[s] ([B, V] float32 holding bf16 values).
    -> tokens [S, B] (and the logits the hook was handed, before it overwrote them)."""
    cfg, lm = _model(device, lib, V)
    temp = TEMP[k] if temp is None else temp
    toks, seen, it = [], [], iter(batches)

    def on_logits(lg):
        assert lg.shape == (B, 1, 1, V) and lg.dtype == torch.bfloat16
        if record_logits:
            seen.append(lg.view(torch.int16).cpu().clone())
        rows = torch.from_numpy(next(it))
        back = rows.to(torch.bfloat16)
        assert torch.equal(back.float(), rows), "a crafted row is not a bf16 row"
        lg[:, 0, 0, :] = back.to(lg.device)

    gen = LMGen(lm, use_sampling=mode != "d", temp=0.9, temp_text=temp, top_k=AUDIO_TOP_K, top_k_text=0 if mode == "c" else max(k, 1),
                seed=seed, support_out_of_sync=True, on_text_logits_hook=on_logits, on_text_hook=lambda t: toks.append(t.cpu().clone()))
    rng = np.random.default_rng(3)
    with gen.streaming(B):
        for s in range(len(batches)):
            codes = torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device)
            if mode == "b":
                gen.step_with_taps(codes, noise=torch.from_numpy(noise[s]))
            else:
                gen.step(codes)
    assert len(toks) == len(batches)
    out = torch.stack(toks).numpy()
    return (out, seen) if record_logits else out


def supplied_noise(k, S, seed):
    """[S, B, 1 + dep_q, kmax] Exp(1) draws for mode (b), as the parity taps take them."""
    kmax = max(AUDIO_TOP_K, k, 1)
    return np.random.default_rng(1000 + seed).exponential(1.0, (S, B, 1 + tiny_lm_config().dep_q, kmax)).astype(np.float32)


def reference(mode, x, k, temp, seed, step, b, noise):
    if mode == "a":
        return ref_fast(x, k, temp, seed, step, b)
    if mode == "b":
        return ref_ranked(x, k, temp, noise[step, b, 0])
    if mode == "c":
        return ref_full(x, temp, seed, step, b)
    return int(np.argmax(x)), True                        # (d) greedy: the first maximum


def craft(V, k, mode, seed):
    """The batches of one engine: every family of families_for(k, mode), one row per (step, session) slot; a row the tie rule
    refuses is drawn again from the next seed.  -> (batches [S][B, V], expected tokens [S, B], family names [S][B])."""
    temp = TEMP[0 if mode == "c" else k]
    fams = families_for(k, mode)
    S = len(fams) // B
    noise = supplied_noise(k, S, seed) if mode == "b" else None
    batches, want, names = [], np.zeros((S, B), np.int64), []
    for s in range(S):
        rows, slot_names = [], []
        for b in range(B):
            fam = fams[s * B + b]
            ctx = {"gumbel": None, "mode": mode, "temp": temp}
            if mode == "a" and fam is plateau_on_the_draws:
                ctx["gumbel"] = -np.log(-np.log(uniform_fast(seed, s, b, np.arange(V))))
            for attempt in range(50):
                rng = np.random.default_rng([V, k, seed, s, b, attempt])
                if mode == "b" and attempt:               # the supplied draws belong to the row: the next seed draws them again too
                    noise[s, b] = rng.exponential(1.0, noise[s, b].shape).astype(np.float32)
                if attempt >= 6:                          # device draws that tie for every row of this shape (all-equal logits)
                    fam = bland
                x = fam(V, k, rng, ctx)
                assert x.shape == (V,) and x.dtype == np.float32 and not np.isnan(x).any()
                tok, decided = reference(mode, x, k, temp, seed, s, b, noise)
                dropped["rows"] += 1
                if decided:
                    break
                dropped["regenerated"] += 1
            else:
                raise AssertionError(f"{fam.__name__}: no decided row in 50 seeds")
            rows.append(x)
            slot_names.append(fam.__name__)
            want[s, b] = tok
        batches.append(np.stack(rows))
        names.append(slot_names)
    return batches, want, names, noise


def check_drop_rate(seed=77):
    """The generator's own condition, over every (V, k, mode) the two test files run (no engine involved; one engine's 24-32
    rows are too few to hold a 2 % bound, and the test workers split the cases between them): at most 2 % of the generated rows
    may be refused by the tie rule."""
    dropped["rows"] = dropped["regenerated"] = 0
    for V in VOCABS:
        for mode, ks in (("a", KS), ("b", KS), ("c", (25,)), ("d", (25,))):
            for k in ks:
                craft(V, k, mode, seed)
    rate = dropped["regenerated"] / max(1, dropped["rows"])
    print(f"sampler rows: {dropped['rows']} generated, {dropped['regenerated']} refused by the tie rule ({100 * rate:.2f} %)")
    assert rate <= 0.02, f"the tie rule refused {100 * rate:.2f} % of the crafted rows"
    return rate


def check_crafted(device, lib, V, k, mode, seed=77):
    """Modes: (a) top-k + device RNG against the float64 reference, (b) supplied noise against the float64 rank-indexed reference
    AND oracle.lm_oracle.sample_token, (c) top_k = 0 against the float64 reference AND the fp32 full-multinomial rule, (d) greedy.
    Equality on every row.  (a) and (c) also establish the step counter: the engine's tokens must match the reference at counter
    == steps since `streaming()` and must NOT all match at the counters either side of it."""
    temp = TEMP[0 if mode == "c" else k]
    batches, want, names, noise = craft(V, k, mode, seed)
    got = run_engine(device, lib, V, k, mode, batches, seed, noise=noise)
    bad = [(s, b, names[s][b], int(got[s, b]), int(want[s, b])) for s in range(len(batches)) for b in range(B) if got[s, b] != want[s, b]]
    assert not bad, f"V={V} k={k} mode ({mode}): (step, session, family, engine's token, reference's) {bad}"
    if mode == "b":
        from oracle.lm_oracle import sample_token
        for s, rows in enumerate(batches):
            tt = sample_token(rows, True, temp, k, noise[s, :, 0])
            for b in range(B):
                if oracle_ranked_is_unambiguous(rows[b], k, temp):
                    assert int(tt[b]) == int(got[s, b]), f"V={V} k={k} step {s} session {b} ({names[s][b]}): the oracle's rule gives {int(tt[b])}, the engine {int(got[s, b])}"
    if mode == "c":
        for s, rows in enumerate(batches):
            for b in range(B):
                assert oracle_full(rows[b], temp, seed, s, b) == int(got[s, b]), (V, s, b, names[s][b])
    if mode in "ac" and (k > 1 or mode == "c"):
        for off in (-1, 1):                               # the convention is discovered, not assumed: the neighbours must fail
            same = all(reference(mode, batches[s][b], k, temp, seed, s + off, b, noise)[0] == got[s, b]
                       for s in range(len(batches)) for b in range(B) if s + off >= 0)
            assert not same, f"the tokens also match Philox step counter = step {off:+d}: the check does not pin the counter"
    return len(batches) * B


# ---- the two ends of the draw ---------------------------------------------------------------------------------------------------------
# (seed, step, session, entry) whose Philox word gives the largest u (top 24 bits all ones: the clamped draw, 1 - 2^-24) and the
# smallest (top 24 bits zero: 2^-25), found by search_extreme_draws() below; fast path: word (i & 3) at counter (step, session,
# i >> 2), full multinomial: word 0 at (step, session, i).  The tests recompute every word and assert it.
EXTREME_DRAWS = {
    ("a", 1000, "hi"): (19787, 1, 0, 546), ("a", 1000, "lo"): (631, 2, 3, 595),
    ("a", 2048, "hi"): (4886, 1, 0, 1272), ("a", 2048, "lo"): (318, 1, 2, 1441),
    ("a", 8192, "hi"): (1126, 1, 0, 2243), ("a", 8192, "lo"): (215, 2, 1, 6398),
    ("a", 32000, "hi"): (649, 1, 0, 11917), ("a", 32000, "lo"): (31, 1, 3, 12824),
    ("c", 0, "hi"): (4886, 1, 0, 318), ("c", 0, "lo"): (566, 2, 3, 603),          # entry < 1000: one pair serves every vocabulary
}


def search_extreme_draws(mode, V, want, steps=(1, 2), sessions=4, seeds=range(1, 400000)):
    """want: "hi" (top 24 bits all ones; searched at step 1, session 0, where the regression row needs it) or "lo" (all zero)."""
    idx = np.arange(V // 4 if mode == "a" else V)
    for seed in seeds:
        for step in ((1,) if want == "hi" else steps):
            for b in range(1 if want == "hi" else sessions):
                w = philox4_words(seed, step, b, idx)
                w = w.reshape(-1) if mode == "a" else w[:, 0]
                hit = (w >> np.uint64(8)) == (0xFFFFFF if want == "hi" else 0)
                if hit.any():
                    return seed, step, b, int(np.nonzero(hit)[0][0])
    raise AssertionError("nothing found")


def word_of(mode, seed, step, b, i) -> int:
    w = philox4_words(seed, step, b, np.array([i >> 2 if mode == "a" else i]))[0]
    return int(w[i & 3] if mode == "a" else w[0])


def check_extreme_draw(device, lib, V, mode, which):
    """A set member sits on the entry with the largest (smallest) possible u, and the logits are chosen so that exactly this
    draw decides: with the largest u the entry wins from well below the others, with the smallest it loses from well above."""
    seed, step, b, i = EXTREME_DRAWS[(mode, V if mode == "a" else 0, which)]
    assert word_of(mode, seed, step, b, i) >> 8 == (0xFFFFFF if which == "hi" else 0)
    k, temp = 25, 0.8
    rng = np.random.default_rng([V, step, i])
    others = np.setdiff1d(_scatter(V, k, rng, must=[i]), [i])[:k - 1]
    u = (uniform_fast if mode == "a" else uniform_entry)(seed, step, b, others)
    g2 = float(np.max(-np.log(-np.log(u))))                                  # the best draw among the others, all at logit 0
    g = -np.log(-np.log(1 - 2.0 ** -24)) if which == "hi" else -np.log(-np.log(2.0 ** -25))     # 16.64 / -2.85
    d = (g - g2 - 1.0) if which == "hi" else (g2 - g - 1.0)                     # i sits d below (above) the others
    assert d > 0.5
    x = np.full(V, -np.inf, np.float32)
    x[others] = 0.0
    x[i] = bf16((-d if which == "hi" else d) * temp)
    batches = [np.stack([bland(V, k, np.random.default_rng([s, r]), None) for r in range(B)]) for s in range(step + 1)]
    batches[step][b] = x
    ref = (lambda row, s_, b_: ref_fast(row, k, temp, seed, s_, b_)) if mode == "a" else (lambda row, s_, b_: ref_full(row, temp, seed, s_, b_))
    tok, decided = ref(x, step, b)
    assert decided and (tok == i) == (which == "hi"), (tok, i, d, g2)
    got = run_engine(device, lib, V, k, mode, batches, seed, temp=temp)
    assert int(got[step, b]) == tok, f"V={V} mode ({mode}) {which}: engine {int(got[step, b])}, reference {tok} (entry {i})"


# ---- u == 1.0: the regression row ---------------------------------------------------------------------------------------------------
# (seed, entry) at step 1, session 0, site 0 whose Philox word has its top 24 bits all ones: ((r >> 8) + 0.5) * 2^-24 rounds to
# 1.0f there, -log(u) is 0 and the entry's score on the fast path +inf whatever its logit (on the other paths -logf(1.0f) = -0.0f
# and p / q = -inf: the entry can never win)
ALL_ONES = {key[:2]: (v[0], v[3]) for key, v in EXTREME_DRAWS.items() if key[2] == "hi"}


def check_u_is_never_one(device, lib, V, mode):
    """k = 25, temp = 1: 24 entries at +24, the entry on the all-ones word at -24, the rest -inf.  With u strictly inside (0, 1)
    that entry scores at most -24 + 16.7 and cannot beat 24 - 2.9: the token must not be it."""
    seed, i = ALL_ONES[(mode, V if mode == "a" else 0)]
    assert i < V and word_of(mode, seed, 1, 0, i) >> 8 == 0xFFFFFF
    rng = np.random.default_rng(V)
    x = np.full(V, -np.inf, np.float32)
    x[np.setdiff1d(_scatter(V, 26, rng), [i])[:24]] = 24.0
    x[i] = -24.0
    batches = [np.stack([bland(V, 25, np.random.default_rng([s, r]), None) for r in range(B)]) for s in range(2)]
    batches[1][0] = x
    got = run_engine(device, lib, V, 25, mode, batches, seed, temp=1.0)
    tok, decided = (ref_fast(x, 25, 1.0, seed, 1, 0) if mode == "a" else ref_full(x, 1.0, seed, 1, 0))
    assert decided and tok != i
    assert int(got[1, 0]) != i, f"V={V} mode ({mode}): entry {i} (logit -24, word {word_of(mode, seed, 1, 0, i):#x}) beat 24 entries at +24"
    assert int(got[1, 0]) == tok
    if mode == "c":
        # on this path the same u == 1.0f shows the other way round: -logf(1.0f) is -0.0f and p / -0.0f = -inf, so the entry could
        # never win.  The mirrored row - it alone at +24, 24 entries at -24 - must pick it (24 + 16.6 against at most -24 + 16.7)
        y = np.where(np.isfinite(x), -x, x).astype(np.float32)
        batches[1][0] = y
        tok, decided = ref_full(y, 1.0, seed, 1, 0)
        assert decided and tok == i
        got = run_engine(device, lib, V, 25, mode, batches, seed, temp=1.0)
        assert int(got[1, 0]) == i, f"V={V} mode (c): entry {i} at +24 on the all-ones word lost to {int(got[1, 0])}"


# ---- fresh streams -----------------------------------------------------------------------------------------------------------------------
def check_repeat_streams(device, lib, V, k=25, seed=77, runs=3):
    """The fast path alone: the same crafted batches on three fresh streams - the tokens and the logits handed to the hook (the
    model's own, before the overwrite) must be bit-identical."""
    batches, want, names, _ = craft(V, k, "a", seed)
    first = run_engine(device, lib, V, k, "a", batches, seed, record_logits=True)
    assert np.array_equal(first[0], want)
    for r in range(1, runs):
        tok, seen = run_engine(device, lib, V, k, "a", batches, seed, record_logits=True)
        assert np.array_equal(tok, first[0]), f"run {r}: tokens differ between two streams fed the same rows"
        assert all(torch.equal(x, y) for x, y in zip(seen, first[1])), f"run {r}: the text logits differ between two streams"
