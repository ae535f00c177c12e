"""Nucleus (top-p) sampling (lm_kernels.h k_sample_nucleus), shared by the simulator and the GPU tests.

The rule: entries ordered by (logit descending, index ascending), P = softmax(x / temp); rank r is in the nucleus iff the mass of
the ranks before it is <= p.  The engine forms the masses in fp32 in its own (fixed) order, the reference in a sequential fp32
cumsum, the restatement here in float64: the three can part only where a prefix mass lies within summation error of p.  So
`nucleus_sizes` gives the prefix sizes under p - DELTA and p + DELTA, and a row is held to a token only where the float64 winner
over both prefixes is the same, decided token (sampler_cases.MARGIN).  DELTA = 2^-10: the engine's hierarchical sum has at most
about 50 dependent additions of non-negative terms that total <= 1 - an error of about 3e-6, 300 times less.

The harness is sampler_cases': `on_text_logits_hook` overwrites the text logits, `on_text_hook` sees the token; the row families,
`uniform_fast`, `_winner` and MARGIN are imported from there.
"""
from __future__ import annotations

import json
import zlib
from dataclasses import replace
from pathlib import Path

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config
from moshi_amd.lm import LMGen, LMModel, SessionSampling
from tests import sampler_cases as sc
from tests.lm_cases import cached_lm_state_dict

B = sc.B
DELTA = 2.0 ** -10
PS = (0.05, 0.3, 0.5, 0.8, 0.9, 0.95, 0.99, 1.0)
TEMP = 0.8
SEED = 77
GOLDEN = Path(__file__).resolve().parent / "golden" / "top_p.json"
DYADIC_SHAPES = ((1000, 512), (2048, 2048), (8192, 8192), (32000, 16384))
WINDOW_WALK = (32000, 4096)          # the same construction at magnitude 2^-95, half of it negative: see window_walk_row
stats = {"rows": 0, "regenerated": 0}


# ---- the rule in float64 ----------------------------------------------------------------------------------------------------------------
def order_of(x: np.ndarray) -> np.ndarray:
    return np.lexsort((np.arange(len(x)), -x.astype(np.float64)))


def nucleus_sizes(x: np.ndarray, temp: float, p: float, delta: float = DELTA):
    """(n_lo, n_hi): the sizes of the prefix of the (-value, index) order whose preceding mass is <= p - delta / <= p + delta
    (delta = 0: the rule itself, for rows whose sums are exact).  Rank 0 always counts.  Entries whose probability is 0 in fp32
    are not counted (the reference's recorder cannot see them, and whether they are members is unspecified: they cannot win)."""
    o = order_of(x)
    z = x[o].astype(np.float64) / temp
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - z[0])
    pr = e / e.sum()
    before = np.concatenate([[0.0], np.cumsum(pr)[:-1]])
    seen = pr >= 2.0 ** -149
    n_lo = int(np.count_nonzero((before <= p - delta) & seen))
    n_hi = int(np.count_nonzero((before <= p + delta) & seen))
    return max(n_lo, 1), max(n_hi, 1)


def winner(x, n, temp, seed, step, a):
    """(token, decided) of the float64 draw over the first n members: x / temp - ln(-ln u), sampler_cases.uniform_fast."""
    m = order_of(x)[:n]
    with np.errstate(divide="ignore"):
        return sc._winner(m, x[m].astype(np.float64) / temp - np.log(-np.log(sc.uniform_fast(seed, step, a, m))))


def expected(x, temp, p, seed, step, a):
    """(token, used, n_lo, n_hi): a row is used iff both winners are decided and the same token."""
    n_lo, n_hi = nucleus_sizes(x, temp, p)
    t0, d0 = winner(x, n_lo, temp, seed, step, a)
    t1, d1 = (t0, d0) if n_hi == n_lo else winner(x, n_hi, temp, seed, step, a)
    return t0, bool(d0 and d1 and t0 == t1), n_lo, n_hi


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def family_row(fam, V, rng, temp):
    """A row of one of sampler_cases' families (crafted for k = 25; the softmax variant of sparse_huge, which stays finite / temp)."""
    return fam(V, 25, rng, {"gumbel": None, "mode": "b", "temp": temp})


def dyadic_row(V, m, seed, scale=1.0):
    """m equal finite logits (a power of two of them) over sampler_cases' edge indices, -inf elsewhere: every probability is 1 / m and
    every partial sum is exact in any order."""
    rng = np.random.default_rng([V, m, seed])
    x = np.full(V, -np.inf, np.float32)
    at = sc._scatter(V, m, rng) if m < V else np.arange(V)
    x[at] = np.float32(scale)
    return x, np.sort(at)


def window_walk_row(V, m, seed):
    """The nucleus boundary more than eight high bytes under the maximum: m / 2 logits at +2^-95 (key high byte 0x90) and m / 2 at
    -2^-95 (high byte 0x6F: 33 high bytes lower).  In fp32 - and in float64 to 1e-28 - every probability is 1 / m, so the dyadic
    rule applies: the nucleus is the first floor(p m) + 1 entries of the (-value, index) order, and for p > 1 / 2 its boundary lies
    among the negative entries, four window steps down."""
    rng = np.random.default_rng([V, m, seed, 1])
    x = np.full(V, -np.inf, np.float32)
    at = np.sort(sc._scatter(V, m, rng))
    pos = np.sort(rng.choice(at, m // 2, replace=False))
    x[at] = np.float32(-2.0 ** -95)
    x[pos] = np.float32(2.0 ** -95)
    return x, order_of(x)[:m]


def dyadic_ps(m):
    return (0.25, 0.5 + 1.0 / (2 * m), 0.75 - 1.0 / (2 * m), 1.0 - 1.0 / m, 1.0)


def dyadic_size(p, m):
    return min(int(np.floor(p * m)) + 1, m)


def crc(x: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(x, np.float32).tobytes())


# ---- the fixture: the rule pinned on the reference's sample_token ------------------------------------------------------------------------
def fixture_rows():
    """(kind, name, V, seed, temp, p, row) of every fixture row, regenerated from its seed: every family at the four vocabularies
    with the p list, and the dyadic rows."""
    fams = list(dict.fromkeys(sc.FAMILIES))
    for V in sc.VOCABS:
        for fi, fam in enumerate(fams):
            for pi, p in enumerate(PS):
                seed = 1000 * fi + pi
                temp = (0.7, 1.0)[(fi + pi) & 1]
                yield "family", fam.__name__, V, seed, temp, p, family_row(fam, V, np.random.default_rng([V, seed]), temp)
    for V, m in DYADIC_SHAPES:
        for p in dyadic_ps(m):
            yield "dyadic", str(m), V, 5, 1.0, p, dyadic_row(V, m, 5)[0]
    V, m = WINDOW_WALK
    for p in dyadic_ps(m):
        yield "dyadic", f"walk{m}", V, 5, 1.0, p, window_walk_row(V, m, 5)[0]


def check_fixture():
    """The float64 restatement brackets the nucleus size the reference's sample_token(x, True, temp, 0, p) handed to its
    multinomial, on every fixture row; on the dyadic rows it equals it, and equals floor(p m) + 1."""
    fx = json.loads(GOLDEN.read_text())
    rows = list(fixture_rows())
    assert len(rows) == len(fx["rows"]) and len(rows) > 600
    worst = 0
    for (kind, name, V, seed, temp, p, x), g in zip(rows, fx["rows"]):
        assert [kind, name, V, seed, temp, p] == g[:6], (g, kind, name, V, seed, temp, p)
        assert crc(x) == g[7], f"{name} V={V} seed={seed}: the regenerated row is not the recorded one"
        n_lo, n_hi = nucleus_sizes(x, temp, p)
        assert 1 <= n_lo <= g[6] <= n_hi, f"{name} V={V} temp={temp} p={p}: the reference kept {g[6]}, the bracket is [{n_lo}, {n_hi}]"
        worst = max(worst, n_hi - n_lo)
        if kind == "dyadic":
            m = int(name.replace("walk", ""))
            assert nucleus_sizes(x, temp, p, 0.0) == (g[6], g[6]) and g[6] == dyadic_size(p, m), (name, V, p, g[6])
    return len(rows), worst


# ---- the harness --------------------------------------------------------------------------------------------------------------------------
def run(device, lib, V, batches, seed=SEED, temp=TEMP, top_p_text=0.0, top_k_text=25, session_top_p=False, settings=None, per_row=None,
        steps=None, greedy=False):
    """One engine of B sessions, one fresh stream; step s samples site 0 from batches[s] ([B, V] float32 holding bf16 values).
    settings[b]: SessionSampling or None; per_row[b]: (top_p, top_p_text) or None, set through set_session_top_p.  -> tokens [S, B]."""
    cfg, lm = sc._model(device, lib, V)
    toks, it = [], iter(batches)

    def on_logits(lg):
        rows = torch.from_numpy(next(it))
        back = rows.to(torch.bfloat16)
        assert torch.equal(back.float(), rows), "a crafted row is not a bf16 row"
        lg[:, 0, 0, :] = back.to(lg.device)

    gen = LMGen(lm, use_sampling=not greedy, temp=0.9, temp_text=temp, top_k=sc.AUDIO_TOP_K, top_k_text=top_k_text, seed=seed,
                support_out_of_sync=True, on_text_logits_hook=on_logits, on_text_hook=lambda t: toks.append(t.cpu().clone()),
                top_p_text=top_p_text, session_top_p=session_top_p)
    rng = np.random.default_rng(3)
    with gen.streaming(B):
        if settings is not None and any(s is not None for s in settings):
            gen.set_session_sampling([s or SessionSampling() for s in settings], mask=[s is not None for s in settings])
        for b, v in enumerate(per_row or []):
            if v is not None:
                gen.set_session_top_p(b, *v)
        for s in range(len(batches) if steps is None else steps):
            gen.step(torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device))
    return torch.stack(toks).numpy()


# ---- 2. crafted rows, token for token ------------------------------------------------------------------------------------------------------
def row_seed(V, s, b, attempt):
    """The Philox seed of the row in slot (s, b): every row is its session's own (a SessionSampling entry set before the step), so a
    regenerated row brings new draws with its new logits."""
    return 100000 * (sc.VOCABS.index(V) + 1) + 1000 * s + 100 * b + attempt


def craft(V, temp=TEMP):
    """Every family of sampler_cases.FAMILIES once per p of PS, one row per (step, session) slot.  p, temp and the seed are the ROW's
    own: the session gets a SessionSampling entry before the step, so its draws are Philox(seed = row_seed, counter (the session's
    offset = step, site 0, entry)) whatever its slot.  A row the two-sided rule does not use is regenerated - same family, same p -
    from the next seed, logits and draws alike.  -> (batches, p [S, B], seeds [S, B], expected token [S, B], n_lo, n_hi, names)."""
    slots = [(fam, p) for fam in dict.fromkeys(sc.FAMILIES) for p in PS[:-1]]
    slots += [(sc.bland, 1.0), (sc.peaked, 1.0), (sc.plateau_wide, 1.0), (sc.coarse_grid, 1.0)]
    while len(slots) % B:
        slots.append((sc.bland, PS[len(slots) % 7]))
    S = len(slots) // B
    batches, ps, want = [], np.zeros((S, B)), np.zeros((S, B), np.int64)
    seeds, lo, hi, names = np.zeros((S, B), np.int64), np.zeros((S, B), np.int64), np.zeros((S, B), np.int64), []
    for s in range(S):
        rows, nm = [], []
        for b in range(B):
            fam, p = slots[s * B + b]
            for attempt in range(50):
                seed = row_seed(V, s, b, attempt)
                x = family_row(fam, V, np.random.default_rng([V, seed]), temp)
                tok, used, n_lo, n_hi = expected(x, temp, p, seed, s, 0)
                stats["rows"] += 1
                if used:
                    break
                stats["regenerated"] += 1
            else:
                raise AssertionError(f"{fam.__name__}: no used row in 50 seeds")
            rows.append(x)
            nm.append(fam.__name__)
            ps[s, b], seeds[s, b], want[s, b], lo[s, b], hi[s, b] = p, seed, tok, n_lo, n_hi
        batches.append(np.stack(rows))
        names.append(nm)
    return batches, ps, seeds, want, lo, hi, names


def check_regeneration_rate():
    """One run = all vocabularies together: at most 2 % of the rows may be regenerated (no engine involved)."""
    stats["rows"] = stats["regenerated"] = 0
    for V in sc.VOCABS:
        craft(V)
    rate = stats["regenerated"] / max(1, stats["rows"])
    print(f"nucleus rows: {stats['rows']} generated, {stats['regenerated']} regenerated ({100 * rate:.2f} %)")
    assert stats["rows"] >= 500
    assert rate <= 0.02, f"the two-sided rule refused {100 * rate:.2f} % of the crafted rows"
    return rate


def run_own_rows(device, lib, V, batches, ps, seeds, ks=None, temp=TEMP):
    """The crafted batches on one stream with the nucleus samplers.  Before step s every session gets a SessionSampling entry with
    the row's seed: top_p_text = ps[s, b] where ks is None, else top_k_text = ks[s, b] and no nucleus - the same per-session draws
    in both forms."""
    cfg, lm = sc._model(device, lib, V)
    toks, at = [], [0]

    def on_logits(lg):
        lg[:, 0, 0, :] = torch.from_numpy(batches[at[0]]).to(torch.bfloat16).to(lg.device)

    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=temp, top_k=sc.AUDIO_TOP_K, top_k_text=25, seed=SEED, support_out_of_sync=True,
                on_text_logits_hook=on_logits, on_text_hook=lambda t: toks.append(t.cpu().clone()), session_top_p=True)
    rng = np.random.default_rng(3)
    with gen.streaming(B):
        for s in range(len(batches)):
            at[0] = s
            gen.set_session_sampling([SessionSampling(temp=0.9, temp_text=temp, top_k=sc.AUDIO_TOP_K, seed=int(seeds[s, b]),
                                                      top_k_text=25 if ks is None else int(ks[s, b]),
                                                      top_p_text=float(ps[s, b]) if ks is None else 0.0) for b in range(B)])
            gen.step(torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device))
    return torch.stack(toks).numpy()


def check_crafted(device, lib, V, against_top_k=True):
    batches, ps, seeds, want, lo, hi, names = craft(V)
    got = run_own_rows(device, lib, V, batches, ps, seeds)
    bad = [(s, b, names[s][b], float(ps[s, b]), int(lo[s, b]), int(hi[s, b]), int(got[s, b]), int(want[s, b]))
           for s in range(len(batches)) for b in range(B) if got[s, b] != want[s, b]]
    assert not bad, f"V={V}: (step, session, family, p, n_lo, n_hi, engine's token, expected) {bad}"
    # the counter is discovered, not assumed: the tokens must not all match at the offsets either side of the step
    for off in (-1, 1):
        same = all(expected(batches[s][b], TEMP, ps[s, b], int(seeds[s, b]), s + off, 0)[0] == got[s, b]
                   for s in range(len(batches)) for b in range(B) if s + off >= 0)
        assert not same, f"the tokens also match the session offset {off:+d}: the check does not pin the counter"
    if against_top_k:
        # engine against engine: where the nucleus has exactly n <= 256 members, top_k_text = n on the same stream gives the same token
        # (on every such row; the others run with top_k_text = 25 and are not compared)
        exact = (lo == hi) & (lo <= 256) & (lo < V)
        assert np.count_nonzero(exact) >= 2 * B
        with_k = run_own_rows(device, lib, V, batches, ps, seeds, np.where(exact, lo, 25))
        diff = [(s, b, int(lo[s, b]), int(got[s, b]), int(with_k[s, b])) for s in range(len(batches)) for b in range(B)
                if exact[s, b] and got[s, b] != with_k[s, b]]
        assert not diff, f"V={V}: (step, session, n, token with top_p, token with top_k = n) {diff}"
    return len(batches) * B


# ---- 3. large nuclei on exact sums ------------------------------------------------------------------------------------------------------------
def check_dyadic(device, lib, V, m, draws=64, walk=False):
    """Over `draws` seeded draws per p (B rows x draws / B steps), every token lies in the exact prefix, and the float64 winner over
    that prefix is the engine's token wherever MARGIN decides it."""
    x, members = window_walk_row(V, m, 5) if walk else dyadic_row(V, m, 5)
    order = order_of(x)[:m]
    S = max(1, draws // B)
    batches = [np.stack([x] * B) for _ in range(S)]
    decided = 0
    for p in dyadic_ps(m):
        n = dyadic_size(p, m)
        assert nucleus_sizes(x, 1.0, p, 0.0) == (n, n)
        got = run(device, lib, V, batches, temp=1.0, top_p_text=p)
        inside = set(order[:n].tolist())
        for s in range(S):
            for b in range(B):
                assert int(got[s, b]) in inside, f"V={V} m={m} p={p} step {s} row {b}: token {int(got[s, b])} is outside the first {n} entries"
                tok, d = winner(x, n, 1.0, SEED, s, b)
                if d:
                    decided += 1
                    assert int(got[s, b]) == tok, f"V={V} m={m} p={p} step {s} row {b}: engine {int(got[s, b])}, float64 winner {tok}"
        if n < m:       # the control: some draw of the full set lands outside the prefix, so the check above can fail
            assert any(winner(x, m, 1.0, SEED, s, b)[0] not in inside for s in range(S) for b in range(B))
    assert decided >= S * B * len(dyadic_ps(m)) // 2
    return decided


# ---- 4. properties on a free-running model -----------------------------------------------------------------------------------------------------
def _codes(cfg, n, steps, device, seed=9):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, cfg.card, (n, cfg.n_q - cfg.dep_q, 1))).to(device) for _ in range(steps)]


def stream(gen, n, codes, between=None):
    out = []
    with gen.streaming(n):
        for s, c in enumerate(codes):
            if between is not None:
                between(gen, s)
            o = gen.step(c)
            out.append(np.full((n, 1 + gen.lm_model.dep_q), -2, np.int64) if o is None else o[:, :, 0].cpu().numpy())
    return np.stack(out)


def tiny_model(device, lib, max_batch=B, cfg=None, **kw):
    cfg = cfg or tiny_lm_config()
    if "max_rows" not in kw:
        kw["max_batch"] = max_batch
    return cfg, LMModel(cached_lm_state_dict(cfg, 21), cfg, device=device, lib=lib, **kw)


def check_tiny_p_is_greedy(device, lib, cfg=None, steps=12, n=3):
    """top_p = top_p_text = 1e-6: the nucleus is the argmax alone, at every site - the sampling stream equals the greedy stream."""
    cfg, lm = tiny_model(device, lib, n, cfg)
    codes = _codes(cfg, n, steps, device)
    a = stream(LMGen(lm, use_sampling=True, temp=0.9, temp_text=0.8, seed=5, top_p=1e-6, top_p_text=1e-6), n, codes)
    g = stream(LMGen(lm, use_sampling=False), n, codes)
    k = stream(LMGen(lm, use_sampling=True, temp=0.9, temp_text=0.8, seed=5), n, codes)
    assert (a >= 0).any() and np.array_equal(a, g), "top_p = 1e-6 does not equal the greedy stream"
    assert not np.array_equal(k, g), "the top-k stream equals the greedy one as well: nothing shown"




def check_enabled_zero_is_today(device, lib, steps=8, n=3):
    """top_p = 0 on an enabled handle: the tokens of a handle that is not enabled, whose launch list names the parent's samplers."""
    cfg, lm = tiny_model(device, lib, n)
    codes = _codes(cfg, n, steps, device)
    lists = {}

    def grab(name):
        def between(gen, s):
            if s == steps - 1:
                lists[name] = gen.launch_list()
        return between
    off = stream(LMGen(lm, use_sampling=True, seed=5), n, codes, grab("off"))
    on = stream(LMGen(lm, use_sampling=True, seed=5, session_top_p=True), n, codes, grab("on"))
    assert (off >= 0).any() and np.array_equal(off, on)
    k_off = [k for _, k in lists["off"] if "k_sample" in k]
    k_on = [k for _, k in lists["on"] if "k_sample" in k]
    assert len(k_off) == len(k_on) == 1 + cfg.dep_q
    assert set(k_off) == {"k_sample"}, k_off                                # the parent's samplers, by the name its launch list gives them
    assert set(k_on) == {"k_sample_nucleus"}, k_on
    assert [k for _, k in lists["off"] if "k_sample" not in k] == [k for _, k in lists["on"] if "k_sample" not in k]


def check_taps(device, lib, steps=5, n=3, seed=77, top_p=0.9, top_p_text=0.8):
    """Every site's token recomputed from the logits taps by the two-sided rule (the shape of lm_cases.check_topk_device_rng)."""
    cfg, lm = tiny_model(device, lib, n)
    temp, temp_text = 0.9, 0.8
    gen = LMGen(lm, use_sampling=True, temp=temp, temp_text=temp_text, top_k=20, top_k_text=10, seed=seed, support_out_of_sync=True,
                top_p=top_p, top_p_text=top_p_text)
    used = [0, 0]

    def pick(logits, t, p, step, site, got):
        for b in range(n):
            x = logits[b].astype(np.float32)
            tok, ok, n_lo, n_hi = expected(x, t, p, seed, step, site * n + b)
            used[1] += 1
            if ok:
                used[0] += 1
                assert int(got[b]) == tok, f"step {step} site {site} row {b}: engine {int(got[b])}, expected {tok} (nucleus {n_lo}..{n_hi})"
    prev = None
    rng = np.random.default_rng(1)
    with gen.streaming(n):
        for s in range(steps):
            codes = rng.integers(0, cfg.card, (n, cfg.n_q - cfg.dep_q, 1))
            out, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device))
            out, tl, al = out.cpu().numpy()[:, :, 0], tl.cpu().numpy(), al.cpu().numpy()
            if prev is not None:      # the ring returns text and codebook 0 one step late (delays 0), the others at once (delays 1)
                pick(prev[0], temp_text, top_p_text, s - 1, 0, out[:, 0])
                pick(prev[1][:, 0], temp, top_p, s - 1, 1, out[:, 1])
                for kq in range(1, cfg.dep_q):
                    pick(al[:, kq], temp, top_p, s, 1 + kq, out[:, 1 + kq])
            prev = (tl, al)
    assert used[0] >= used[1] * 3 // 4, used


def check_slot_independence(device, lib, steps=10):
    """A session with its own seed and its own top_p yields the same tokens in slot 0 and in the last slot."""
    cfg, lm = tiny_model(device, lib, B)
    codes = _codes(cfg, B, steps, device)
    own = SessionSampling(temp=0.85, temp_text=0.75, top_k=30, top_k_text=12, seed=2024, top_p=0.7, top_p_text=0.6)

    def at(slot):
        def between(gen, s):
            if s == 0:
                gen.set_session_sampling(own, mask=[b == slot for b in range(B)])
        perm = list(range(B))
        perm[0], perm[slot] = perm[slot], perm[0]
        return stream(LMGen(lm, use_sampling=True, seed=5, session_top_p=True), B, [c[perm] for c in codes], between)[:, slot]
    a, z = at(0), at(B - 1)
    assert (a >= 0).any() and np.array_equal(a, z), "the session's tokens depend on its slot"

    def between_k(gen, s):
        if s == 0:
            gen.set_session_sampling(replace(own, top_p=0.0, top_p_text=0.0), mask=[b == 0 for b in range(B)])
    k = stream(LMGen(lm, use_sampling=True, seed=5, session_top_p=True), B, codes, between_k)[:, 0]
    assert not np.array_equal(a, k), "the session's top_p changed no token: nothing shown"


def check_change_and_snapshot(device, lib, steps=12):
    """Changing one session's top_p between two steps changes no other session's tokens and leaves the launch list alone; a snapshot
    taken before the change and restored after it reproduces the original continuation bit for bit."""
    cfg, lm = tiny_model(device, lib, B)
    codes = _codes(cfg, B, steps, device)
    state = {}
    mk = lambda: LMGen(lm, use_sampling=True, seed=5, top_p=0.9, top_p_text=0.9)     # noqa: E731
    base = stream(mk(), B, codes)

    def between(gen, s):
        if s == 6:
            state["snap"] = gen.get_streaming_state()
            state["list"] = gen.launch_list()
            gen.set_session_top_p(2, 0.05, 0.05)
        if s == 9:
            assert gen.launch_list() == state["list"], "changing a session's top_p changed the launch list"
            gen.set_streaming_state(state["snap"])
    changed = stream(mk(), B, codes[:9] + codes[6:9], between)
    others = [b for b in range(B) if b != 2]
    assert np.array_equal(changed[:9, others], base[:9, others]), "another session's tokens changed"
    assert not np.array_equal(changed[6:9, 2], base[6:9, 2]), "the session's own tokens did not change: nothing shown"
    assert np.array_equal(changed[9:12], base[6:9]), "a restored stream does not continue bit for bit"

    def cleared(gen, s):
        if s == 3:
            gen.set_session_top_p(2, 0.05, 0.05)
        if s == 6:
            gen.reset_streaming(torch.tensor([b == 5 for b in range(B)]))      # a reset keeps the values
        if s == 8:
            gen.clear_session_top_p(2)
    c = stream(mk(), B, codes, cleared)
    assert np.array_equal(c[:3], base[:3]) and np.array_equal(c[:, others][:6], base[:, others][:6])


def check_guided_addresses_sessions(device, lib, V=1000, steps=6):
    """cfg_coef != 1: 4 sessions run 8 model rows; the nucleus table is indexed by session."""
    batches = [np.stack([sc.bland(V, 25, np.random.default_rng([V, s, b, 6]), None) for b in range(4)]) for s in range(steps)]
    cfg, lm = sc._model(device, lib, V)
    toks, at = [], [0]

    def on_logits(lg):
        lg[:, 0, 0, :] = torch.from_numpy(batches[at[0]]).to(torch.bfloat16).to(lg.device)
    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=TEMP, top_k=sc.AUDIO_TOP_K, top_k_text=25, seed=SEED, cfg_coef=2.0,
                cfg_is_no_text=True, on_text_logits_hook=on_logits, on_text_hook=lambda t: toks.append(t.cpu().numpy().copy()),
                session_top_p=True)
    rng = np.random.default_rng(3)
    with gen.streaming(4):
        gen.set_session_top_p(3, 0.0, 0.3)
        for s in range(steps):
            at[0] = s
            gen.step(torch.from_numpy(rng.integers(0, cfg.card, (4, cfg.n_q - cfg.dep_q, 1))).to(device))
    n_used = 0
    for s in range(steps):
        for b in range(4):
            if b == 3:
                tok, ok, _, _ = expected(batches[s][b], TEMP, 0.3, SEED, s, b)
            else:
                tok, ok = sc.reference("a", batches[s][b], 25, TEMP, SEED, s, b, None)
            if ok:
                n_used += 1
                assert int(toks[s][b]) == tok, (s, b, int(toks[s][b]), tok)
    assert n_used >= steps * 3


def check_many_rows(device, lib, steps=6, n=70):
    """One case on a many-row handle: the nucleus stream with p = 1e-6 is the greedy stream there too."""
    cfg, lm = tiny_model(device, lib, n, max_rows=n)
    codes = _codes(cfg, n, steps, device)
    a = stream(LMGen(lm, use_sampling=True, seed=5, top_p=1e-6, top_p_text=1e-6), n, codes)
    g = stream(LMGen(lm, use_sampling=False), n, codes)
    assert (a >= 0).any() and np.array_equal(a, g)


def check_repeat(device, lib, V=2048, runs=3):
    """A repeated stream on one handle is bit-identical: the crafted nucleus rows (every family, every p) and a free-running model."""
    batches, ps, seeds, want, lo, hi, names = craft(V)
    first = run_own_rows(device, lib, V, batches, ps, seeds)
    assert np.array_equal(first, want)
    for r in range(1, runs):
        assert np.array_equal(run_own_rows(device, lib, V, batches, ps, seeds), first), f"run {r}: tokens differ between two streams fed the same rows"
    cfg, lm = tiny_model(device, lib, B)
    codes = _codes(cfg, B, 6, device)
    free = [stream(LMGen(lm, use_sampling=True, seed=5, top_p=0.9, top_p_text=0.8), B, codes) for _ in range(runs)]
    assert all(np.array_equal(f, free[0]) for f in free[1:])


def check_duplex(device, lib, B_=3, steps=8, join_every=4):
    """The duplex pipeline with nucleus rows is bit-identical to the serial loop."""
    from tests import duplex_cases as dc
    from tests.batcher_cases import tiny_pair
    mimi, lm, mcfg, lcfg = tiny_pair(device, lib, B_)
    dev = torch.device(device)
    rng = np.random.default_rng(7)
    frames = [(0.1 * rng.standard_normal((B_, 1, mcfg.frame_size))).astype(np.float32) for _ in range(steps)]
    ones = np.ones(B_, bool)
    m1 = ones.copy(); m1[B_ - 1] = False
    r1 = np.zeros(B_, bool); r1[0] = True
    events = {4: [("mask", m1)], 6: [("mask", ones), ("reset", r1)]}
    runs = []
    for fn, p in ((dc._serial, 0.8), (lambda *a: dc._pipelined(*a, join_every), 0.8), (dc._serial, 0.0)):
        gen = LMGen(lm, use_sampling=True, temp=0.8, temp_text=0.7, top_k=5, top_k_text=5, seed=99, top_p=p, top_p_text=p, session_top_p=True)
        with mimi.streaming(B_), gen.streaming(B_):
            if p:
                gen.set_session_top_p(1, 0.5, 0.95)
            runs.append(fn(mimi, gen, frames, events, dev))
    serial, piped, plain = runs
    n_valid = 0
    for t, (x, y) in enumerate(zip(serial, piped)):
        assert (x is None) == (y is None), f"frame {t}: None pattern differs"
        if x is None:
            continue
        n_valid += 1
        assert np.array_equal(x[0], y[0]), f"frame {t}: tokens differ"
        assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), f"frame {t}: PCM differs"
    assert n_valid >= steps - 2
    assert any(x is not None and not np.array_equal(x[0], z[0]) for x, z in zip(serial, plain)), "top_p changed no token: nothing shown"


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def check_refusals(device, lib, V=1000):
    """Every refusal raises the mapped exception, changes nothing and leaves the handle usable."""
    import ctypes as C

    import pytest
    cfg, lm = sc._model(device, lib, V)
    L, h = lm._lib, lm._handle
    codes = torch.zeros(B, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=device)
    noise = torch.ones(B, 1 + cfg.dep_q, 250)

    def values():
        a, t = C.c_float(-1), C.c_float(-1)
        L.check(L.mmi_lm_top_p(h, C.byref(a), C.byref(t)))
        return round(a.value, 6), round(t.value, 6)
    # out-of-domain values: the constructors, the dataclass and the C calls
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            LMGen(lm, top_p=bad)
        with pytest.raises(ValueError):
            LMGen(lm, top_p_text=bad)
        with pytest.raises(ValueError):
            SessionSampling(top_p=bad).validate()
        with pytest.raises(ValueError):
            SessionSampling(top_p_text=bad).validate()
    # a handle that is not enabled refuses a non-zero value (MMI_ERR_STATE) and keeps 0
    L.check(L.mmi_lm_set_top_p(h, 0.0, 0.0))
    L.check(L.mmi_lm_enable_nucleus(h, 0))
    with pytest.raises(RuntimeError):
        L.check(L.mmi_lm_set_top_p(h, 0.5, 0.0))
    assert values() == (0.0, 0.0)
    L.check(L.mmi_lm_enable_nucleus(h, 1))
    L.check(L.mmi_lm_set_top_p(h, 0.5, 0.25))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            L.check(L.mmi_lm_set_top_p(h, bad, 0.5))
        with pytest.raises(ValueError):
            L.check(L.mmi_lm_set_top_p(h, 0.5, bad))
    assert values() == (0.5, 0.25)                                          # refused calls changed nothing; the values stay until changed
    with pytest.raises(RuntimeError):
        L.check(L.mmi_lm_enable_nucleus(h, 0))                              # not while the handle's values are positive
    with pytest.raises(RuntimeError):
        L.check(L.mmi_lm_set_row_top_p(h, 0, 0.5, 0.5, None))               # not streaming
    with pytest.raises(RuntimeError):
        L.check(L.mmi_lm_clear_row_top_p(h, 0, None))
    # a stream WITHOUT the kernels: per-session values are refused, supplied noise is accepted
    plain = LMGen(lm, use_sampling=True, seed=1)
    with plain.streaming(B):
        assert values() == (0.0, 0.0)                                       # an LMGen states the handle's values at its start
        with pytest.raises(RuntimeError):
            plain.set_session_top_p(0, 0.5, 0.5)
        with pytest.raises(RuntimeError):
            plain.clear_session_top_p(0)
        with pytest.raises(RuntimeError):
            plain.set_session_sampling(SessionSampling(seed=3, top_p=0.5))
        plain.step_with_taps(codes, noise=noise)                            # the refused set_session_sampling activated no row
        with pytest.raises(RuntimeError):
            L.check(L.mmi_lm_enable_nucleus(h, 1))                          # MMI_ERR_STATE while streaming
        with pytest.raises(RuntimeError):
            L.check(L.mmi_lm_set_top_p(h, 0.0, 0.0))
        plain.step(codes)
    # a stream WITH the kernels and every value 0: noise is accepted until a session's value is positive
    gen = LMGen(lm, use_sampling=True, seed=1, session_top_p=True)
    with gen.streaming(B):
        gen.step_with_taps(codes, noise=noise)
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError):
                gen.set_session_top_p(1, bad, 0.0)
            with pytest.raises(ValueError):
                gen.set_session_top_p(1, 0.0, bad)
        for bad in (-1, B):
            with pytest.raises(ValueError):
                gen.set_session_top_p(bad, 0.5, 0.5)
        gen.step_with_taps(codes, noise=noise)                              # refused calls changed nothing
        gen.set_session_top_p(5, 0.0, 0.5)
        with pytest.raises(NotImplementedError):
            gen.step_with_taps(codes, noise=noise)
        gen.step(codes)                                                     # the handle is still usable
        gen.clear_session_top_p(5)
        gen.step_with_taps(codes, noise=noise)
    # the handle's own value is positive: noise is refused from the first step
    gen = LMGen(lm, use_sampling=True, seed=1, top_p=0.9)
    with gen.streaming(B):
        assert values() == (0.9, 0.0)
        with pytest.raises(NotImplementedError):
            gen.step_with_taps(codes, noise=noise)
        gen.step(codes)
    plain = LMGen(lm, use_sampling=True, seed=1)
    with plain.streaming(B):
        plain.step_with_taps(codes, noise=noise)


def check_batcher_channels(device, lib):
    """A channel's own top_p: the tokens of greedy for p = 1e-6, for the channel's life; the row returns to the batcher's values at
    the step after the close; a refused nucleus part leaves no channel open."""
    import pytest

    from moshi_amd.batcher import SessionBatcher
    from tests.batcher_cases import tiny_pair
    slots, n = 3, 9
    mimi, lm, mcfg, lcfg = tiny_pair(device, lib, slots)
    F = mcfg.frame_size
    pcm = (0.3 * np.random.default_rng(5).standard_normal((n, F))).astype(np.float32)

    def frames(b, ch):
        out = []
        for f in range(n):
            b.push(ch, pcm[f])
            b.step()
            while (fr := b.pop(ch)) is not None:
                out.append(fr[1])
        return np.stack(out)
    with SessionBatcher(mimi, lm, slots, use_sampling=True, seed=11) as b:
        with pytest.raises(RuntimeError):
            b.open(sampling=SessionSampling(seed=4, top_p=0.5))
        assert b.used_slots == 0
        ch = b.open()
        with pytest.raises(RuntimeError):
            b.set_channel_top_p(ch, 0.5, 0.5)                               # a batcher without the nucleus samplers
        frames(b, ch)
    with SessionBatcher(mimi, lm, slots, use_sampling=False) as b:
        greedy = frames(b, b.open())
    with SessionBatcher(mimi, lm, slots, use_sampling=True, seed=11, session_top_p=True) as b:
        with pytest.raises(ValueError):
            b.open(sampling=SessionSampling(seed=4, top_p=1.5))
        assert b.used_slots == 0
        ch = b.open()
        b.set_channel_top_p(ch, 1e-6, 1e-6)
        with pytest.raises(ValueError):
            b.set_channel_top_p(ch, 2.0, 0.0)
        tiny = frames(b, ch)
        b.close(ch)
        again = frames(b, b.open())                                          # the same slot, without values of its own
        own = frames(b, b.open(sampling=SessionSampling(use_sampling=True, seed=11, top_p=1e-6, top_p_text=1e-6)))
    with SessionBatcher(mimi, lm, slots, use_sampling=True, seed=11, session_top_p=True) as b:     # the same history without the values
        ch = b.open()
        frames(b, ch)
        b.close(ch)
        plain = frames(b, b.open())
    assert np.array_equal(tiny, greedy) and np.array_equal(own, greedy)
    assert np.array_equal(again, plain), "the slot's next channel still samples with the closed channel's top_p"
    assert not np.array_equal(plain, greedy)
