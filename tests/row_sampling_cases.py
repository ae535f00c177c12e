"""Per-session sampling (mmi_lm_set_row_sampling: lm_kernels.h k_sample / k_lm_commit, lm_engine.hip, batcher.hip), shared by
the simulator and the GPU tests.  The mechanism is tests/sampler_cases.py's: `on_text_logits_hook` injects crafted bf16 rows just
before k_sample runs at the text site, `on_text_hook` reads (and in some cases replaces) the token.

The references are sampler_cases' float64 ones.  An ACTIVE row draws from Philox keyed by its own seed at counter (the row's
stream offset, a = site = 0, entry), so its reference is `sc.reference(mode, x, k_b, temp_b, seed_b, step=offset, b=0, ...)`;
an inactive row keeps the handle's seed and counter (step since `streaming()`, a = row index).  The two logit adjustments are
restated below in numpy (fp32 operations in the stated order, then bf16 through `sc.bf16`), and the text history is replayed on
the Python side from the committed tokens: the engine's tokens must EQUAL the reference on the adjusted rows at every step, which
they can only do if its ring holds what the replay holds.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config
from moshi_amd.lm import LMGen, SessionSampling
from tests import sampler_cases as sc

B = sc.B
G = dict(temp_text=0.8, top_k_text=25, seed=77)             # the handle's own settings in every engine below
PAD, EOP = 3, 0                                             # existing_text_padding_id, end_of_text_padding_id
MIXED_STEPS = 12


# ---- the two adjustments, restated ----------------------------------------------------------------------------------------------------
def adjust(x: np.ndarray, hist, s: SessionSampling, start_id: int) -> np.ndarray:
    """x: one bf16 row as float32.  hist: every committed text token of the row, oldest first (specials included: the ring
    skips them here).  Repetition penalty over the distinct tokens among the newest `repetition_context` of the last 64 non-
    special ones, then the pad bias on sampling rows."""
    x = x.copy()
    V = len(x)
    ring = [t for t in hist if t not in (PAD, EOP, start_id)][-64:]
    if s.repetition_context > 0 and s.repetition_penalty != 1.0:
        p = np.float32(s.repetition_penalty)
        for t in set(ring[-s.repetition_context:]):
            if 0 <= t < V:
                l = np.float32(x[t])
                x[t] = sc.bf16(l / p if l >= 0 else l * p)
    if s.use_sampling and s.temp_text > 0 and s.pad_mult != 0.0 and PAD < V:
        prod = np.float32(np.float32(s.pad_mult) * np.float32(s.temp_text))
        x[PAD] = sc.bf16(np.float32(x[PAD]) + prod)
    return x


def mode_of(s: SessionSampling) -> str:
    if not s.use_sampling or not s.temp_text > 0:
        return "d"
    return "c" if s.top_k_text == 0 else "a"


def expect(x, s: SessionSampling | None, step, row, offset):
    """(token, decided) of one row: its own settings and counter when active, else the handle's."""
    if s is None:
        return sc.reference("a", x, G["top_k_text"], G["temp_text"], G["seed"], step, row, None)
    return sc.reference(mode_of(s), x, max(s.top_k_text, 1), s.temp_text, s.seed, offset, 0, None)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def run(device, lib, V, batches, settings, steps=None, replace_tok=None, between=None, codes=None, use_rows=True, cfg_kwargs=None,
        record=None):
    """One engine of B sessions, one fresh stream.  batches[s]: [B, V] crafted rows (None: the model's own logits).  settings[b]:
    SessionSampling or None (inactive).  replace_tok(step, tokens[B]) -> tokens or None.  between(gen, step) runs before step.
    -> (text tokens [S, B], step outputs [S, B, 1 + dep_q] with -2 before the delay is over)."""
    cfg, lm = sc._model(device, lib, V)
    S = steps if steps is not None else len(batches)
    toks, outs, at = [], [], [0]

    def on_logits(lg):
        if record is not None:
            record.append(lg.view(torch.int16).cpu().clone())
        rows = torch.from_numpy(batches[at[0]])
        back = rows.to(torch.bfloat16)
        assert torch.equal(back.float(), rows), "a crafted row is not a bf16 row"
        lg[:, 0, 0, :] = back.to(lg.device)

    def on_text(t):
        if replace_tok is not None:
            r = replace_tok(at[0], t.cpu().numpy().copy())
            if r is not None:
                t.copy_(torch.from_numpy(np.asarray(r, np.int64)).to(t.device))
        toks.append(t.cpu().clone())

    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=G["temp_text"], top_k=sc.AUDIO_TOP_K, top_k_text=G["top_k_text"],
                seed=G["seed"], support_out_of_sync=True, on_text_logits_hook=on_logits if batches is not None else None,
                on_text_hook=on_text, **(cfg_kwargs or {}))
    rng = np.random.default_rng(3)
    with gen.streaming(B):
        if use_rows and any(s is not None for s in settings):
            gen.set_session_sampling([s or SessionSampling() for s in settings], mask=[s is not None for s in settings])
        for s in range(S):
            at[0] = s
            if between is not None:
                between(gen, s)
            c = codes[s] if codes is not None else rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))
            out = gen.step(torch.from_numpy(np.asarray(c)).to(device))
            outs.append(np.full((B, 1 + cfg.dep_q), -2, np.int64) if out is None else out[:, :, 0].cpu().numpy())
    return torch.stack(toks).numpy(), np.stack(outs)


# ---- 1. mixed rows --------------------------------------------------------------------------------------------------------------------
def mixed_settings(V):
    """Rows 0-4: their own (temp_text, top_k_text, seed) from sampler_cases.KS / TEMP; 5: greedy; 6: top_k_text = 0; 7: inactive."""
    rot = sc.VOCABS.index(V) if V in sc.VOCABS else 0
    out = []
    for b in range(5):
        k = sc.KS[(b + rot) % len(sc.KS)]
        out.append(SessionSampling(temp=0.9, temp_text=sc.TEMP[k], top_k=sc.AUDIO_TOP_K, top_k_text=k, seed=1000 + 17 * b + V))
    out.append(SessionSampling(use_sampling=False, seed=5))
    out.append(SessionSampling(temp=0.9, temp_text=sc.TEMP[0], top_k=sc.AUDIO_TOP_K, top_k_text=0, seed=4242))
    out.append(None)
    return out


def craft_mixed(V, seed=91, steps=MIXED_STEPS, stats=None):
    """-> (batches [S][B, V], expected tokens [S, B], family names).  Admission by sampler_cases' rule: a row whose two best
    scores are closer than MARGIN is regenerated from the next seed."""
    settings = mixed_settings(V)
    batches, want, names = [], np.zeros((steps, B), np.int64), []
    for s in range(steps):
        rows, nm = [], []
        for b in range(B):
            st = settings[b]
            mode = "a" if st is None else mode_of(st)
            k = G["top_k_text"] if st is None else max(st.top_k_text, 1)
            temp = G["temp_text"] if st is None else st.temp_text
            fams = sc.families_for(k, mode)
            fam = fams[(s * B + b) % len(fams)]
            ctx = {"gumbel": None, "mode": mode, "temp": temp}
            if mode == "a" and fam is sc.plateau_on_the_draws:
                u = sc.uniform_fast(G["seed"], s, b, np.arange(V)) if st is None else sc.uniform_fast(st.seed, s, 0, np.arange(V))
                ctx["gumbel"] = -np.log(-np.log(u))
            for attempt in range(50):
                rng = np.random.default_rng([V, seed, s, b, attempt])
                if attempt >= 6:
                    fam = sc.bland
                x = fam(V, k, rng, ctx)
                tok, decided = expect(x, st, s, b, s)
                if stats is not None:
                    stats["rows"] += 1
                if decided:
                    break
                if stats is not None:
                    stats["regenerated"] += 1
            else:
                raise AssertionError(f"{fam.__name__}: no decided row in 50 seeds")
            rows.append(x)
            nm.append(fam.__name__)
            want[s, b] = tok
        batches.append(np.stack(rows))
        names.append(nm)
    return batches, want, names


def check_mixed_drop_rate():
    """CPU only, the reference alone: at most 2 % of the generated rows may be refused by the tie rule (over the four
    vocabularies: one engine's 96 rows are too few to hold a 2 % bound)."""
    stats = {"rows": 0, "regenerated": 0}
    for V in sc.VOCABS:
        craft_mixed(V, stats=stats)
    rate = stats["regenerated"] / stats["rows"]
    assert rate <= 0.02, f"the tie rule refused {100 * rate:.2f} % of {stats['rows']} crafted rows"
    return rate


def check_mixed_rows(device, lib, V):
    batches, want, names = craft_mixed(V)
    got, _ = run(device, lib, V, batches, mixed_settings(V))
    bad = [(s, b, names[s][b], int(got[s, b]), int(want[s, b])) for s in range(len(batches)) for b in range(B) if got[s, b] != want[s, b]]
    assert not bad, f"V={V}: (step, row, family, engine's token, reference's) {bad}"
    # the counter of an active row is its offset and a = site: neither the neighbouring counters nor a = row index may fit
    st = mixed_settings(V)
    for b in (1, 2):
        for off, a in ((-1, 0), (1, 0), (0, b)):
            same = all(sc.reference("a", batches[s][b], st[b].top_k_text, st[b].temp_text, st[b].seed, s + off, a, None)[0] == got[s, b]
                       for s in range(len(batches)) if s + off >= 0)
            assert not same, f"row {b}: the tokens also match counter {off:+d} / a = {a}: the check does not pin the draw counter"


# ---- 7. repeat streams -----------------------------------------------------------------------------------------------------------------
def check_repeat_streams(device, lib, V, runs=3):
    batches, want, _ = craft_mixed(V)
    first_seen = []
    first = run(device, lib, V, batches, mixed_settings(V), record=first_seen)
    assert np.array_equal(first[0], want)
    for r in range(1, runs):
        seen = []
        tok, out = run(device, lib, V, batches, mixed_settings(V), record=seen)
        assert np.array_equal(tok, first[0]) and np.array_equal(out, first[1]), f"run {r}: tokens differ between two streams fed the same rows"
        assert all(torch.equal(x, y) for x, y in zip(seen, first_seen)), f"run {r}: the text logits differ between two streams"


# ---- 2. slot independence ---------------------------------------------------------------------------------------------------------------
PERM = [3, 7, 0, 5, 1, 6, 2, 4]           # row r of the second run holds session PERM[r]


def _all_active(V):
    st = mixed_settings(V)
    st[7] = SessionSampling(temp=0.9, temp_text=0.8, top_k=sc.AUDIO_TOP_K, top_k_text=25, seed=31337, repetition_penalty=1.5,
                            repetition_context=8, pad_mult=0.5)
    return st


def check_slot_independence(device, lib, V, crafted=True, active=True, steps=10):
    """Same per-session logits, user codes and settings, once in row order and once permuted across rows: with every row active
    each session's text and audio tokens are bit-identical.  active=False is the negative control: with the handle's counter
    (a = site * B + row) a session's draws move with its slot, so at least one token differs."""
    cfg, _ = sc._model(device, lib, V)
    rng = np.random.default_rng(V + 1)
    batches = [np.stack([sc.bland(V, 25, np.random.default_rng([V, s, b]), None) for b in range(B)]) for s in range(steps)] if crafted else None
    codes = [rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1)) for _ in range(steps)]
    st = _all_active(V) if active else [None] * B
    t1, o1 = run(device, lib, V, batches, st, steps=steps, codes=codes)
    pb = [x[PERM] for x in batches] if crafted else None
    t2, o2 = run(device, lib, V, pb, [st[p] for p in PERM], steps=steps, codes=[c[PERM] for c in codes])
    same = all(np.array_equal(t1[:, PERM[r]], t2[:, r]) and np.array_equal(o1[:, PERM[r]], o2[:, r]) for r in range(B))
    if active:
        for r in range(B):
            assert np.array_equal(t1[:, PERM[r]], t2[:, r]), f"session {PERM[r]}: text tokens differ between row {PERM[r]} and row {r}"
            assert np.array_equal(o1[:, PERM[r]], o2[:, r]), f"session {PERM[r]}: output tokens differ between row {PERM[r]} and row {r}"
        assert (o1 >= 0).any()
    else:
        assert not same, "inactive rows: every session sampled the same tokens in another slot - the control shows nothing"


# ---- 3. a one-session stream of today ---------------------------------------------------------------------------------------------------
def check_equals_one_session_lmgen(device, lib, steps=12):
    """LMGen(seed=s, temp...) on one session == the same values set through set_session_sampling on a one-session stream whose
    handle has other settings: rng[1] starts at 0 and a = site when B = 1."""
    cfg = tiny_lm_config()
    _, lm = sc._model(device, lib, cfg.text_card)
    rng = np.random.default_rng(9)
    codes = [torch.from_numpy(rng.integers(0, cfg.card, (1, cfg.n_q - cfg.dep_q, 1))).to(device) for _ in range(steps)]
    vals = dict(temp=0.85, temp_text=0.65, top_k=30, top_k_text=12, seed=2024)

    def stream(gen, own):
        out = []
        with gen.streaming(1):
            if own:
                gen.set_session_sampling(SessionSampling(**vals))
            for c in codes:
                o = gen.step(c)
                out.append(None if o is None else o.cpu().numpy())
        return out
    a = stream(LMGen(lm, use_sampling=True, **vals), False)
    b = stream(LMGen(lm, use_sampling=True, temp=0.5, temp_text=1.1, top_k=5, top_k_text=50, seed=1), True)
    c = stream(LMGen(lm, use_sampling=True, temp=0.5, temp_text=1.1, top_k=5, top_k_text=50, seed=1), False)
    assert sum(o is not None for o in a) >= steps - cfg.max_delay - 1
    for s, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), f"step {s}: {x} != {y}"
    assert any(x is not None and not np.array_equal(x, z) for x, z in zip(a, c)), "the other handle settings give the same tokens: nothing shown"


# ---- 4. repetition penalty and pad bias -------------------------------------------------------------------------------------------------
def _row(V, base, put):
    x = np.full(V, base, np.float32)
    for i, v in put.items():
        x[i] = v
    assert np.array_equal(sc.bf16(x), x)
    return x


def penalty_script(V, steps):
    """-> (settings, batches, replace_tok, decisive) - every row of the batch is one scenario; `decisive` lists (step, row)
    where the adjusted row's token must differ from the unadjusted row's."""
    A, Bt, Ct = 10, V - 2, 500
    greedy = dict(use_sampling=False)
    st = [
        SessionSampling(**greedy, repetition_penalty=2.0, repetition_context=8),                   # 0: positive logits
        SessionSampling(**greedy, repetition_penalty=2.0, repetition_context=8),                   # 1: negative logits, seen twice
        SessionSampling(**greedy, repetition_penalty=2.0, repetition_context=2),                   # 2: just outside the context, specials between
        SessionSampling(**greedy, repetition_penalty=2.0, repetition_context=64),                  # 3: the ring wraps (hooked tokens)
        SessionSampling(**greedy, repetition_penalty=1.0, repetition_context=8),                   # 4: penalty = 1: no-op
        SessionSampling(**greedy, repetition_penalty=2.0, repetition_context=0, pad_mult=4.0),     # 5: context = 0 no-op; pad bias ignored when greedy
        SessionSampling(temp_text=0.5, top_k_text=2, seed=7, pad_mult=40.0),                       # 6: pad lifted into the top-k set
        SessionSampling(temp_text=0.7, top_k_text=25, seed=8, repetition_penalty=1.5, repetition_context=16, pad_mult=-1.0),   # 7: sampled, all at once
    ]
    batches = []
    for s in range(steps):
        rows = [None] * B
        rows[0] = _row(V, -8.0, {A: 4.0, Bt: 3.0})                          # s0 A; s1 A -> 2: B; s2 A 2, B 1.5: A; ...
        rows[1] = _row(V, -8.0, {A: -1.0, Bt: -1.5, Ct: -3.5})              # s0 A; s1 A -> -2: B; s2 A -2, B -3: A; s3 A seen twice, once: -2 > -3
        # row 2: the hook commits A, PAD, EOP, start, B, Ct (steps 0-5): the newest two non-special entries are B, Ct; A is just outside
        rows[2] = _row(V, -8.0, {A: 4.0, Bt: 4.5, Ct: 5.0, 7: 3.0})
        rows[3] = _row(V, -8.0, {100: 4.0, 102: 3.875, 50: 3.0})
        rows[4] = _row(V, -8.0, {A: 4.0, Bt: 3.0})
        rows[5] = _row(V, -8.0, {A: 4.0, Bt: 3.0, PAD: 3.5})
        rows[6] = _row(V, -30.0, {A: 2.0, Bt: 1.5, PAD: 0.5})               # top-2 = {A, B}; + 40 * 0.5 lifts PAD to 20.5: beyond any draw
        rng = np.random.default_rng([V, s, 7])
        rows[7] = sc.bf16(2.0 * rng.standard_normal(V))
        batches.append(np.stack(rows))
    hooked2 = {0: A, 1: PAD, 2: EOP, 3: V, 4: Bt, 5: Ct}                    # V = text_card = the start id

    def replace_tok(step, t):
        if step in hooked2:
            t[2] = hooked2[step]
        t[3] = 100 + step                                                   # the history of row 3 is 100, 101, ...
        return t
    # (row 1, step 3: A was seen twice and is penalised once, -2 > -3; an engine that penalised it twice would pick B there)
    decisive = [(1, 0), (1, 1), (6, 2), (6, 6)]
    return st, batches, replace_tok, decisive


def check_penalty_and_pad(device, lib, V, steps=70):
    st, batches, replace_tok, decisive = penalty_script(V, steps)
    got, _ = run(device, lib, V, batches, st, replace_tok=replace_tok)
    hist = [[] for _ in range(B)]
    for s in range(steps):
        for b in range(B):
            x = batches[s][b]
            tok, decided = expect(adjust(x, hist[b], st[b], V), st[b], s, b, s)
            plain, _ = expect(x, st[b], s, b, s)
            if (s, b) in decisive:
                assert decided and tok != plain, f"step {s} row {b}: the adjustment does not decide this case ({tok}, {plain})"
            if b in (4, 5):
                assert tok == plain                                          # the no-ops
            sampled = tok
            if b == 3 or (b == 2 and s <= 5):
                sampled = None                                               # replaced by the hook before it is recorded
            if sampled is not None and decided:
                assert int(got[s, b]) == tok, f"V={V} step {s} row {b}: engine {int(got[s, b])}, reference on the adjusted row {tok}"
            hist[b].append(int(got[s, b]))                                  # what the step committed (after the hook)
    # row 3 reads tokens at every step from the hook: what the SAMPLER picked there is visible in no output, so its decisive
    # step is checked through a second run that stops replacing at step 66
    if steps > 66:
        def replace_until(step, t):
            if step < 66:
                return replace_tok(step, t)
            return None
        got2, _ = run(device, lib, V, batches[:67], st, replace_tok=replace_until)
        h3 = [100 + s for s in range(66)]
        want, decided = expect(adjust(batches[66][3], h3, st[3], V), st[3], 66, 3, 66)
        wrong, _ = expect(adjust(batches[66][3], [100] + h3[-63:], st[3], V), st[3], 66, 3, 66)        # a ring that kept token 100
        assert decided and want == 100 and wrong != want
        assert int(got2[66, 3]) == want, f"V={V}: after 66 tokens the ring still penalises token 100 (engine {int(got2[66, 3])})"
        # row 2 at step 6 in the same run: A (just outside the context of 2) wins un-penalised; the specials in between did not count
        h2 = [10, PAD, EOP, V, V - 2, 500]
        want2, d2 = expect(adjust(batches[6][2], h2, st[2], V), st[2], 6, 2, 6)
        assert d2 and want2 == 10 and int(got2[6, 2]) == want2


# ---- 5. lifecycle ------------------------------------------------------------------------------------------------------------------------
def check_lifecycle(device, lib, V=1000, steps=12):
    """Settings changed between two steps act at the next step with the launch list untouched; a reset empties the ring and keeps
    the settings (and returns the row's counter to 0); clear restores the handle's tokens; a snapshot in mid-stream continues
    token for token."""
    batches = [np.stack([sc.bland(V, 25, np.random.default_rng([V, s, b, 5]), None) for b in range(B)]) for s in range(steps)]
    own = SessionSampling(temp_text=0.6, top_k_text=10, seed=99, repetition_penalty=3.0, repetition_context=32, pad_mult=0.25)
    state = {}
    # rows on which the ring decides.  Row 2 commits OLD at step 5 and, after its reset before step 6, NEW; at step 7 the penalty
    # (96 / 3 = 32 < 48) must hit NEW alone: a ring the reset did not empty would also hold OLD (48 / 3 = 16 < 32) and NEW would
    # win; a row that lost its settings would pick NEW (96) as well.  Row 1 commits T1 at step 7 and is cleared before step 8,
    # where T1 must win un-penalised; a row still on its own settings would pick T1B.  The gaps are far beyond any draw.
    OLD, NEW, T1, T1B = 20, 21, 30, 31
    batches[5][2][OLD] = 96.0
    batches[6][2][NEW] = 96.0
    batches[7][2][NEW], batches[7][2][OLD] = 96.0, 48.0
    batches[7][1][T1] = 96.0
    batches[8][1][T1], batches[8][1][T1B] = 96.0, 48.0
    # an un-hooked stream (the graph-replayed step on the GPU): the launch list is the same before and after, the tokens are not
    cfg, lm = sc._model(device, lib, V)
    gen = LMGen(lm, use_sampling=True, seed=G["seed"])
    codes = torch.from_numpy(np.random.default_rng(1).integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device)
    with gen.streaming(B):
        for _ in range(3):
            gen.step(codes)
        before = gen.launch_list()
        gen.set_session_sampling(own, mask=[b in (1, 2, 4) for b in range(B)])
        for _ in range(3):
            gen.step(codes)
        assert before and gen.launch_list() == before, "changing a row's settings changed the launch list"
        assert not any("k_lm_set_rows" in k for _, k in before)

    def between(gen, s):
        if s == 3:
            gen.set_session_sampling(own, mask=[b in (1, 2, 4) for b in range(B)])
        if s == 6:
            gen.reset_streaming(torch.tensor([b == 2 for b in range(B)]))
        if s == 8:
            gen.clear_session_sampling(mask=[b == 1 for b in range(B)])
            state["snap"] = gen.get_streaming_state()
        if s == 10 and "replay" in state:
            gen.set_streaming_state(state["snap"])
    user = [np.random.default_rng([2, s]).integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1)) for s in range(steps)]
    got, out = run(device, lib, V, batches, [None] * B, between=between, codes=user)
    hist = {1: [], 2: [], 4: []}
    off = {b: 0 for b in range(B)}
    for s in range(steps):
        if s == 6:
            hist[2], off[2] = [], 0
        for b in range(B):
            active = (b in (2, 4) and s >= 3) or (b == 1 and 3 <= s < 8)
            x = batches[s][b]
            if active:
                tok, decided = expect(adjust(x, hist[b], own, V), own, s, b, off[b])
            else:
                tok, decided = expect(x, None, s, b, off[b])
            if decided:
                assert int(got[s, b]) == tok, f"step {s} row {b} ({'own' if active else 'handle'} settings): engine {int(got[s, b])}, reference {tok}"
            if active:
                hist[b].append(int(got[s, b]))
            off[b] += 1
    assert (int(got[5, 2]), int(got[6, 2]), int(got[7, 1])) == (OLD, NEW, T1)
    kept, d_kept = expect(adjust(batches[7][2], [NEW], own, V), own, 7, 2, 1)
    stale, _ = expect(adjust(batches[7][2], [OLD, NEW], own, V), own, 7, 2, 1)
    lost, _ = expect(batches[7][2], None, 7, 2, 7)
    assert d_kept and (kept, stale, lost) == (OLD, NEW, NEW), "the crafted row does not tell the three outcomes apart"
    assert int(got[7, 2]) == OLD, f"after the reset row 2 picked {int(got[7, 2])}: its ring was not emptied, or its settings were lost"
    back, d_back = expect(batches[8][1], None, 8, 1, 8)
    still, _ = expect(adjust(batches[8][1], [T1], own, V), own, 8, 1, 8)
    assert d_back and (back, still) == (T1, T1B)
    assert int(got[8, 1]) == T1, f"after the clear row 1 picked {int(got[8, 1])}: it still samples with its own settings"
    # mid-stream snapshot: restore at step 10 what was saved at step 8 and feed steps 8, 9 again - the same tokens
    state["replay"] = True
    seq = batches[:10] + batches[8:10]
    got2, out2 = run(device, lib, V, seq, [None] * B, between=between, codes=user[:10] + user[8:10])
    assert np.array_equal(got2[:10], got[:10])
    assert np.array_equal(got2[10:12], got[8:10]), "a restored stream does not continue token for token"
    assert np.array_equal(out2[10:12], out[8:10])


def check_guided_addresses_sessions(device, lib, V=1000, steps=6):
    """cfg_coef != 1: 4 sessions run 8 model rows; the table is indexed by session, so session 3's settings act on session 3."""
    batches = [np.stack([sc.bland(V, 25, np.random.default_rng([V, s, b, 6]), None) for b in range(4)]) for s in range(steps)]
    cfg, lm = sc._model(device, lib, V)
    own = SessionSampling(temp_text=0.6, top_k_text=10, seed=123)
    toks, at = [], [0]

    def on_logits(lg):
        lg[:, 0, 0, :] = torch.from_numpy(batches[at[0]]).to(torch.bfloat16).to(lg.device)
    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=G["temp_text"], top_k=sc.AUDIO_TOP_K, top_k_text=G["top_k_text"], seed=G["seed"],
                cfg_coef=2.0, cfg_is_no_text=True, on_text_logits_hook=on_logits, on_text_hook=lambda t: toks.append(t.cpu().numpy().copy()))
    rng = np.random.default_rng(3)
    with gen.streaming(4):
        gen.set_session_sampling(own, mask=[False, False, False, True])
        for s in range(steps):
            at[0] = s
            gen.step(torch.from_numpy(rng.integers(0, cfg.card, (4, cfg.n_q - cfg.dep_q, 1))).to(device))
    for s in range(steps):
        for b in range(4):
            tok, decided = (sc.reference("a", batches[s][b], 10, 0.6, 123, s, 0, None) if b == 3 else
                            sc.reference("a", batches[s][b], G["top_k_text"], G["temp_text"], G["seed"], s, b, None))
            if decided:
                assert int(toks[s][b]) == tok, (s, b, int(toks[s][b]), tok)


def check_refusals(device, lib, V=1000):
    """Every refusal raises the mapped exception and leaves the handle usable."""
    import pytest
    cfg, lm = sc._model(device, lib, V)
    gen = LMGen(lm, use_sampling=True, seed=1)
    codes = torch.zeros(B, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=device)
    ok = SessionSampling(seed=3)
    with pytest.raises(AssertionError):
        gen.set_session_sampling(ok)                                        # not streaming
    with gen.streaming(B):
        for bad, exc in ((replace(ok, top_k=257), NotImplementedError), (replace(ok, top_k_text=300), NotImplementedError),
                         (replace(ok, top_k=-1), ValueError), (replace(ok, repetition_context=65), ValueError),
                         (replace(ok, repetition_context=-1), ValueError), (replace(ok, repetition_penalty=0.0), ValueError),
                         (replace(ok, repetition_penalty=-2.0), ValueError), (replace(ok, temp=float("nan")), ValueError),
                         (replace(ok, pad_mult=float("inf")), ValueError), (replace(ok, temp_text=float("-inf")), ValueError)):
            with pytest.raises(exc):
                gen.set_session_sampling(bad)
            with pytest.raises(exc):
                bad.validate()                                              # the Python restatement agrees with the engine
            # all or nothing: one bad entry among good ones changes no row - supplied noise is still accepted
            with pytest.raises(exc):
                gen.set_session_sampling([ok] * (B - 1) + [bad])
        noise = torch.ones(B, 1 + cfg.dep_q, 250)
        gen.step_with_taps(codes, noise=noise)                              # no row is active: accepted
        gen.set_session_sampling(ok, mask=[b == 5 for b in range(B)])
        with pytest.raises(NotImplementedError):
            gen.step_with_taps(codes, noise=noise)
        gen.step(codes)                                                     # the handle is still usable
        gen.clear_session_sampling()
        gen.step_with_taps(codes, noise=noise)
        with pytest.raises(AssertionError):
            gen.set_session_sampling([ok] * (B - 1))
    with pytest.raises(RuntimeError):
        lib_ = lm._lib
        lib_.check(lib_.mmi_lm_clear_row_sampling(lm._handle, None, None))  # MMI_ERR_STATE outside a stream


def check_end_padding_id_of_the_model(device, lib, V=1000):
    """A checkpoint may move the end-of-padding id (LMConfig.existing_text_end_padding_id): the ring skips THAT id and records
    token 0 like any other.  One greedy row, penalty 2 over the newest 2 entries; the hook commits A, EOP', 0, so the ring holds
    A, 0 and token 7 wins (4 / 2 = 2, 3.5 / 2 = 1.75 < 3); a ring that skipped id 0 would hold A alone and pick token 0."""
    import pytest
    from moshi_amd.lm import LMModel
    from tests.lm_cases import cached_lm_state_dict
    A, EOP2 = 10, 5
    cfg = replace(tiny_lm_config(), text_card=V, existing_text_end_padding_id=EOP2)
    lm = LMModel(cached_lm_state_dict(cfg, 21), cfg, device=device, max_batch=1, lib=lib)
    assert lm.end_of_text_padding_id == EOP2
    x = _row(V, -8.0, {A: 4.0, 0: 3.5, 7: 3.0})
    commits, toks, at = {0: A, 1: EOP2, 2: 0}, [], [0]

    def on_logits(lg):
        lg[:, 0, 0, :] = torch.from_numpy(x).to(torch.bfloat16).to(lg.device)

    def on_text(t):
        toks.append(int(t.cpu().reshape(-1)[0]))
        if at[0] in commits:
            t.fill_(commits[at[0]])
    gen = LMGen(lm, use_sampling=True, seed=1, on_text_logits_hook=on_logits, on_text_hook=on_text)
    codes = torch.zeros(1, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=device)
    with gen.streaming(1):
        with pytest.raises(RuntimeError):                                   # part of the launch list: not while streaming
            lib_ = lm._lib
            lib_.check(lib_.mmi_lm_set_text_end_padding_id(lm._handle, 0))
        gen.set_session_sampling(SessionSampling(use_sampling=False, repetition_penalty=2.0, repetition_context=2))
        for s in range(4):
            at[0] = s
            gen.step(codes)
    assert toks[0] == A and toks[1] == 0, toks                              # un-penalised, then A halved
    assert toks[3] == 7, f"the ring does not hold (A, 0): the sampler picked {toks[3]}"
    with pytest.raises(ValueError):
        lm._lib.check(lm._lib.mmi_lm_set_text_end_padding_id(lm._handle, V + 1))


# ---- the duplex pipeline with active rows ----------------------------------------------------------------------------------------------
def check_duplex_with_active_rows(device, lib, B_=3, steps=8, join_every=4):
    """DuplexStream takes the LMGen it is given; with rows that have their own settings it still runs bit-identically to the
    serial loop: tests/duplex_cases.py's two drivers and its mask / reset events, on streams whose rows are activated here."""
    from tests import duplex_cases as dc
    from tests.batcher_cases import tiny_pair
    own = [SessionSampling(temp=0.7, temp_text=0.6, top_k=20, top_k_text=10, seed=50 + b, repetition_penalty=1.3, repetition_context=16,
                           pad_mult=0.5) for b in range(B_)]
    mimi, lm, mcfg, lcfg = tiny_pair(device, lib, B_)
    dev = torch.device(device)
    rng = np.random.default_rng(7)
    frames = [(0.1 * rng.standard_normal((B_, 1, mcfg.frame_size))).astype(np.float32) for _ in range(steps)]
    ones = np.ones(B_, bool)
    m1 = ones.copy(); m1[B_ - 1] = False
    r1 = np.zeros(B_, bool); r1[0] = True
    events = {4: [("mask", m1)], 6: [("mask", ones), ("reset", r1)]}
    runs = []
    for fn, settings in ((dc._serial, own), (lambda *a: dc._pipelined(*a, join_every), own), (dc._serial, None)):
        gen = LMGen(lm, use_sampling=True, temp=0.8, temp_text=0.7, top_k=5, top_k_text=5, seed=99)
        with mimi.streaming(B_), gen.streaming(B_):
            if settings is not None:
                gen.set_session_sampling(settings)
            runs.append(fn(mimi, gen, frames, events, dev))
    serial, piped, plain = runs
    assert len(serial) == len(piped) == steps
    n_valid = 0
    for t, (x, y) in enumerate(zip(serial, piped)):
        assert (x is None) == (y is None), f"frame {t}: None pattern differs"
        if x is None:
            continue
        n_valid += 1
        assert np.array_equal(x[0], y[0]), f"frame {t}: tokens differ"
        assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), f"frame {t}: PCM differs"
    assert n_valid >= steps - 2
    assert any(x is not None and not np.array_equal(x[0], z[0]) for x, z in zip(serial, plain)), "the rows' own settings changed no token: nothing shown"
    return n_valid


# ---- 6. the batcher ---------------------------------------------------------------------------------------------------------------------
def check_batcher_channels(device, lib):
    """Three channels: one greedy, one seeded, one plain.  The seeded channel's frames are the same whether it is opened first or
    last (another slot); a slot closed and reopened plain samples with the batcher's defaults again."""
    from moshi_amd.batcher import SessionBatcher
    from tests.batcher_cases import tiny_pair
    slots, n = 3, 9
    mimi, lm, mcfg, lcfg = tiny_pair(device, lib, slots)
    F = mcfg.frame_size
    pcm = {c: (0.3 * np.random.default_rng(ord(c)).standard_normal((n, F))).astype(np.float32) for c in "gsp"}
    greedy = SessionSampling(use_sampling=False)
    seeded = SessionSampling(temp=0.8, temp_text=0.7, top_k=50, top_k_text=25, seed=4711, repetition_penalty=1.2, repetition_context=8)

    def session(order, how, reopen_plain=False):
        res = {c: [] for c in order}
        with SessionBatcher(mimi, lm, slots, use_sampling=True, seed=11) as b:
            import pytest
            with pytest.raises(ValueError):
                b.open(sampling=replace(seeded, repetition_context=99))
            assert b.used_slots == 0                                        # a refused open claims no slot
            ch = {c: b.open(sampling=how[c]) for c in order}
            for f in range(n):
                for c in order:
                    b.push(ch[c], pcm[c][f])
                assert b.step() == len(order)
                for c in order:
                    while (fr := b.pop(ch[c])) is not None:
                        res[c].append(fr)
            if reopen_plain:                                                # the seeded channel's slot, reopened without settings
                b.close(ch["s"])
                again = b.open()
                res["again"] = []
                for f in range(n):
                    b.push(again, pcm["p"][f])
                    b.step()
                    while (fr := b.pop(again)) is not None:
                        res["again"].append(fr)
        return res
    how = {"g": greedy, "s": seeded, "p": None}
    first = session("sgp", how)
    last = session("gps", how, reopen_plain=True)
    assert len(first["s"]) == len(last["s"]) > 3
    for i, ((pa, ta), (pb, tb)) in enumerate(zip(first["s"], last["s"])):
        assert np.array_equal(ta, tb) and np.array_equal(pa, pb), f"frame {i}: the seeded channel depends on its slot"
    for (pa, ta), (pb, tb) in zip(first["g"], last["g"]):                   # greedy: slot-independent too
        assert np.array_equal(ta, tb)
    # the plain channel samples with the batcher's settings and counter: alone in slot 0 of a fresh batcher it gives the frames
    # that the reopened slot gives only if that slot is back on the defaults - same slot (2), same counter offset is not given, so
    # compare against a run where the slot's first owner was plain as well
    ref = session("gps", {"g": greedy, "p": None, "s": None}, reopen_plain=True)
    assert len(ref["again"]) == len(last["again"]) > 3
    for i, ((pa, ta), (pb, tb)) in enumerate(zip(ref["again"], last["again"])):
        assert np.array_equal(ta, tb), f"frame {i}: a slot reopened without settings still samples with its last owner's"
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(ref["s"], last["s"])), "seeded and plain give the same tokens: nothing shown"
