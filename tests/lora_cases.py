"""Cases for per-session LoRA adapters kept unmerged next to one base model (`LMModel(adapters=...)`, `load_adapter`,
`LMGen.set_session_adapter`; k_gemm_xp<.., LORA> / <.., LORA_T>, k_pack_lora_slot), shared by the simulator tests
(tests/test_lora_sim.py) and the GPU tests (tests/test_z_lora_gpu.py).

Yardsticks: the reference's own unfused run (tests/golden/lm_lora.npz, written by tests/golden/make_golden_lm_lora.py) for the
network, sums that are exact in fp32 in any order for single linears, and bit equality wherever two runs of the engine must
compute the same thing (slots, neighbours, plain handles, repeat streams)."""
from __future__ import annotations

from dataclasses import replace
from pathlib import Path

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config
from moshi_amd.lm import LMGen, LMModel
from moshi_amd.weights import is_lm_linear_weight, random_lm_state_dict
from oracle.lm_oracle import bf16r, silu
from tests import lm_cases as lc
from tests.lm_cases import _bf16_bits, cached_lm_state_dict
from tests.many_rows_cases import env, linear_sites

GOLDEN = Path(__file__).resolve().parent / "golden"
# the knobs under which a plain handle takes the launch list of an adapter handle minus its shrink launches
UNFUSED = {"MMI_GEMM_LDS": "0", "MMI_GEMM_ONCE": "0", "MMI_NO_NORM_FUSION": "1", "MMI_NO_DEP_ATTN_FUSION": "1", "MMI_NO_DEP_IN_GROUP": "1"}


def adapter_keys(sd):
    return [k[: -len(".weight")] for k in sd if is_lm_linear_weight(k)]


def random_adapter(sd, rank, seed, a_std=0.25, b_std=0.25, only=None):
    """A seeded adapter over every linear of `sd` (or those whose stem passes `only`): lora_A ~ N(0, a_std^2 / in_features),
    lora_B ~ N(0, b_std^2 / rank) - the draw of tests/golden/make_golden_lm_lora.py."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for stem in adapter_keys(sd):
        N, K = sd[stem + ".weight"].shape
        a = (torch.randn(rank, K, generator=g) * (a_std / K ** 0.5)).to(torch.bfloat16)
        b = (torch.randn(N, rank, generator=g) * (b_std / rank ** 0.5)).to(torch.bfloat16)
        if only is None or only(stem):
            out[stem + ".lora_A.weight"], out[stem + ".lora_B.weight"] = a, b
    return out


def rand_codes(cfg, B, steps, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))) for _ in range(steps)]


def run_taps(gen, codes, device, forced=None):
    out = []
    for i, c in enumerate(codes):
        f = None if forced is None else torch.from_numpy(forced[i]).to(device)
        tok, tl, al = gen.step_with_taps(c.to(device), forced_tokens=f)
        out.append((tok.cpu().clone(), tl.cpu().clone(), al.cpu().clone()))
    return out


def same_rows(a, b, rows_a, rows_b, what):
    for s, (x, y) in enumerate(zip(a, b)):
        for t, name in zip(range(3), ("tokens", "text logits", "audio logits")):
            assert torch.equal(x[t][rows_a], y[t][rows_b]), f"{what}: step {s}: {name} differ"


# ---- a. the reference's own unfused run ------------------------------------------------------------------------------------------------------
def check_golden_mixed_slots(device, lib):
    """ONE batch with mixed slots - row i takes slot (i % 3) - 1 - against the reference's three runs (no adapter, adapter 0,
    adapter 1; LoRALinear.forward unfused, modules/lora.py:116-118), every row against the run of its own adapter, teacher-forced
    with that run's tokens.  The golden's adapted rows are far from its base rows (asserted here and by the generator), so the
    comparison fails on an engine that ignores the adapters."""
    g = np.load(GOLDEN / "lm_lora.npz")
    cfg = tiny_lm_config()
    seed, rank, scaling = int(g["seed"][0]), int(g["rank"][0]), float(g["scaling"][0])
    sd = random_lm_state_dict(cfg, seed=seed)
    ads = [random_adapter(sd, rank, int(s), float(g["a_std"][0]), float(g["b_std"][0])) for s in g["adapter_seeds"]]
    codes, tl, al, tt, at = g["codes"], g["text_logits"], g["audio_logits"], g["text_tokens"], g["audio_tokens"]   # [run][step][B]...
    S, B = codes.shape[0], codes.shape[1]
    for run in (1, 2):          # what makes this test fail without the feature
        for s in range(S):
            for b in range(B):
                assert not lc.logits_close(tl[run, s, b], tl[0, s, b], widen=4.0), f"golden run {run} step {s} row {b} is within 4x the gate of the base run"
    lm = LMModel(sd, cfg, device=device, max_batch=B, lib=lib, adapters=(2, rank))
    for j, ad in enumerate(ads):
        lm.load_adapter(j, ad, scaling=scaling)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    run_of = [(i % 3) for i in range(B)]                      # slot + 1 = the golden run
    worst = 0.0
    with gen.streaming(B):
        for i in range(B):
            gen.set_session_adapter(i, run_of[i] - 1 if run_of[i] else None)
        for s in range(S):
            forced = np.stack([np.concatenate([tt[run_of[b], s, b][None], at[run_of[b], s, b]]) for b in range(B)])
            out, etl, eal = gen.step_with_taps(torch.from_numpy(codes[s]).to(device), forced_tokens=torch.from_numpy(forced).to(device))
            etl, eal = etl.cpu().numpy(), eal.cpu().numpy()
            for b in range(B):
                r = run_of[b]
                worst = max(worst, float(np.abs(etl[b] - tl[r, s, b]).max() / (np.abs(tl[r, s, b]).max() + 1e-6)))
                assert lc.logits_close(etl[b], tl[r, s, b]), f"step {s} row {b} (golden run {r}): text logits {np.abs(etl[b] - tl[r, s, b]).max()}"
                a_e, a_o = int(etl[b].argmax()), int(tt[r, s, b])
                assert a_e == a_o or lc.near_tie(tl[r, s, b], a_e, a_o), f"step {s} row {b}: text token {a_e} != {a_o}"
                for k in range(cfg.dep_q):
                    assert lc.logits_close(eal[b, k], al[r, s, b, k]), f"step {s} row {b} cb {k} (golden run {r}): {np.abs(eal[b, k] - al[r, s, b, k]).max()}"
                    a_e, a_o = int(eal[b, k].argmax()), int(at[r, s, b, k])
                    assert a_e == a_o or lc.near_tie(al[r, s, b, k], a_e, a_o), f"step {s} row {b} cb {k}: token {a_e} != {a_o}"
        sites = {site for site, _ in gen.launch_list()}
    assert "L.in_proj.lora" in sites and "dep.lin.lora" in sites and "text_linear.lora" in sites, sorted(sites)
    return worst


# ---- b. exact sums through debug_linear_lora ----------------------------------------------------------------------------------------------------
# Base weights: integers -4..4 times 2^-7.  lora_A rows: exactly 8 nonzeros of +-2^-3, one in every eighth of K (so every wave's
# slice and every K split contributes).  x rows of +-1.  lora_B: integers -4..4 times 2^-4, scaling 2.  Then t = A x is a multiple
# of 1/8 with |t| <= 1 - a bf16 value - and every term of W x (multiples of 2^-7, |sum| <= 4 K 2^-7) and of (2 B) t (multiples of
# 2^-6, |sum| <= r / 2) is a small multiple of 2^-7: every partial sum is exact in fp32 in ANY order (asserted on the float64 sums).
EXACT_ROWS = {16: (1, 16), 32: (1, 16, 17), 64: (1, 16, 17, 33, 64)}


def exact_state_dict(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    sd = dict(cached_lm_state_dict(cfg, seed))
    for key in [k for k in sd if is_lm_linear_weight(k)]:
        sd[key] = (torch.randint(-4, 5, sd[key].shape, generator=g).float() * 2.0 ** -7).to(torch.bfloat16)
    return sd


def exact_adapter(sd, rank, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for stem in adapter_keys(sd):
        N, K = sd[stem + ".weight"].shape
        a = torch.zeros(rank, K)
        for i in range(8):
            lo, hi = i * K // 8, (i + 1) * K // 8
            pos = lo + torch.randint(0, hi - lo, (rank,), generator=g)
            a[torch.arange(rank), pos] = (torch.randint(0, 2, (rank,), generator=g).float() * 2 - 1) * 2.0 ** -3
        out[stem + ".lora_A.weight"] = a.to(torch.bfloat16)
        out[stem + ".lora_B.weight"] = (torch.randint(-4, 5, (N, rank), generator=g).float() * 2.0 ** -4).to(torch.bfloat16)
    return out


def _exact_reference(x64, w64, ads, slots, key, gated, scaling=2.0):
    stem = key[: -len(".weight")]
    h64 = x64 @ w64.T
    bound = np.abs(x64) @ np.abs(w64).T
    for b, sl in enumerate(slots):
        if sl < 0 or ads[sl] is None:
            continue
        A, Bm = ads[sl][stem + ".lora_A.weight"].double().numpy(), ads[sl][stem + ".lora_B.weight"].double().numpy()
        t = A @ x64[b]
        assert np.abs(t).max() <= 1.0 and np.array_equal(t * 8, np.round(t * 8)), "t must be a multiple of 1/8 with |t| <= 1 (a bf16 value)"
        assert np.array_equal(bf16r(t.astype(np.float32)).astype(np.float64), t)
        h64[b] += (scaling * Bm) @ t
        bound[b] += np.abs(scaling * Bm) @ np.abs(t)
    # every partial sum is a multiple of 2^-7 below 2^17 units: exact in fp32 in any order
    assert bound.max() < 2.0 ** 10 and np.array_equal(h64 * 128, np.round(h64 * 128))
    h = bf16r(h64.astype(np.float32))
    if gated:
        H = h.shape[1] // 2
        return bf16r(bf16r(silu(h[:, :H])) * h[:, H:])
    return h


def _compare(out, ref, gated, name):
    """mxfp4_cases._compare: plain linears identical, gated >= 99.9 % identical and everywhere within one bf16 step."""
    same = _bf16_bits(out) == _bf16_bits(ref)
    if gated:
        ulp = np.abs(out - ref) <= np.maximum(np.abs(ref), 1e-30) * 2.0 ** -7
        assert same.mean() >= 0.999 and ulp.all(), f"{name}: gated output {same.mean():.5f} identical, worst {np.abs(out - ref).max()}"
    else:
        assert same.all(), f"{name}: {int((~same).sum())} of {same.size} bf16 outputs differ (first at {np.argwhere(~same)[0]})"


def exact_handle(device, lib, cfg, max_batch, ksplit, seed, max_adapters=4, max_rank=32, ranks=(32, 16, 32, 8)):
    """Slot 0: full rank; slot 1: a rank below max_rank; slot 2: loaded, then unloaded (= none); slot 3: rank 8."""
    sd = exact_state_dict(cfg, seed)
    with env(**({"MMI_GEMM_KSPLIT": ksplit} if ksplit else {})):
        lm = LMModel(sd, cfg, device=device, max_batch=max_batch, lib=lib, adapters=(max_adapters, max_rank))
    ads = [exact_adapter(sd, r, seed + 10 + j) for j, r in enumerate(ranks)]
    for j, ad in enumerate(ads):
        lm.load_adapter(j, ad, scaling=2.0)
    lm.unload_adapter(2)
    ads[2] = None
    return lm, sd, ads


def check_linears_exact(device, lib, max_batch, ksplit=None, seed=41):
    cfg = tiny_lm_config()
    lm, sd, ads = exact_handle(device, lib, cfg, max_batch, ksplit, seed)
    rng = np.random.default_rng(seed)
    checked = split = adapted = 0
    for key, paths in linear_sites(cfg):
        w = sd[key].double().numpy()
        gated = "linear_in" in key
        for path in paths:
            for B in EXACT_ROWS[max_batch]:
                x = rng.choice(np.array([-1.0, 1.0], np.float32), (B, w.shape[1]))
                slots = [int(v) for v in (np.arange(B) + rng.integers(0, 5)) % 5 - 1]          # -1, 0, 1, 2, 3 over the rows
                try:
                    out = lm.debug_linear_lora(key, torch.from_numpy(x), slots, path=path)["out"].float().cpu().numpy()
                except NotImplementedError as e:
                    if path == "splitk" and "does not split" in str(e):      # tiny shapes are not split over K unless forced
                        continue
                    raise
                ref = _exact_reference(x.astype(np.float64), w, ads, slots, key, gated)
                base = _exact_reference(x.astype(np.float64), w, ads, [-1] * B, key, gated)
                _compare(out, ref, gated, f"{key} [{path}] rows={B} max_batch={max_batch} ksplit={ksplit} slots={slots}")
                adapted += int((_bf16_bits(ref) != _bf16_bits(base)).any())
                checked += 1
                split += path == "splitk"
    if ksplit and int(ksplit) > 1:
        assert split >= len(EXACT_ROWS[max_batch]), f"MMI_GEMM_KSPLIT={ksplit}: only {split} split-K cases ran"
    assert adapted >= checked // 2, "the adapters barely change the expected outputs: the case checks nothing"
    return checked


# ---- c. one 7B layer's widths (GPU only) ---------------------------------------------------------------------------------------------------------
def check_7b_layer_shapes(device, lib, seed=7):
    """in_proj (4096 -> 12288), the gated linear_in (4096 -> 2 x 11264) and the split-K linear_out (11264 -> 4096) of one 7B layer,
    four rank-128 adapters, at 32 and 64 rows: the production wave and split-K plans with the tail.  The recipe of b:
    |W x| <= 11264 * 4 * 2^-7 = 352, |(2 B) t| <= 128 / 2 = 64, multiples of 2^-7: below 2^24 units."""
    cfg = replace(tiny_lm_config(), dim=4096, num_heads=32, num_layers=1, hidden_scale=4.125, context=8, text_card=64)
    assert cfg.ffn_hidden == 11264
    lm, sd, ads = exact_handle(device, lib, cfg, 64, None, seed, max_adapters=4, max_rank=128, ranks=(128, 128, 128, 128))
    rng = np.random.default_rng(seed)
    for key, path in (("transformer.layers.0.self_attn.in_projs.0.weight", "plain"), ("transformer.layers.0.gating.linear_in.weight", "plain"),
                      ("transformer.layers.0.gating.linear_out.weight", "splitk")):
        w = sd[key].double().numpy()
        x = rng.choice(np.array([-1.0, 1.0], np.float32), (64, w.shape[1]))
        slots = [int(v) for v in (np.arange(64) % 5) - 1]
        ref = _exact_reference(x.astype(np.float64), w, ads, slots, key, "linear_in" in key)       # once: the 32-row case reads its first rows
        for B in (32, 64):
            out = lm.debug_linear_lora(key, torch.from_numpy(x[:B]), slots[:B], path=path)["out"].float().cpu().numpy()
            _compare(out, ref[:B], "linear_in" in key, f"7B {key} [{path}] rows={B}")


# ---- d. independence ----------------------------------------------------------------------------------------------------------------------------------
def adapter_model(device, lib, cfg, max_batch, seed, slots=3, rank=32, loaded=(0, 1, 2)):
    sd = cached_lm_state_dict(cfg, seed)
    lm = LMModel(sd, cfg, device=device, max_batch=max_batch, lib=lib, adapters=(slots, rank))
    for j in loaded:
        lm.load_adapter(j, random_adapter(sd, rank if j != 1 else rank // 2, 900 + j, 1.0, 1.0), scaling=2.0)
    return lm, sd


def check_slot_independence(device, lib, B=4, steps=3, seed=51):
    """The same session (inputs, adapter, seed) in slot 0 and in the last slot, next to neighbours on other adapters or on none:
    the same tokens and logits, as numbers."""
    cfg = tiny_lm_config()
    lm, sd = adapter_model(device, lib, cfg, B, seed)
    ad = random_adapter(sd, 32, 900, 1.0, 1.0)                 # slot 0's adapter again, for the last slot
    lm.load_adapter(2, ad, scaling=2.0)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    codes = rand_codes(cfg, B, steps, seed)
    with gen.streaming(B):
        gen.set_session_adapter(0, 0); gen.set_session_adapter(1, 1); gen.set_session_adapter(3, 2)
        first = run_taps(gen, codes, device)
    moved = [torch.cat([c[3:4], c[1:3], c[0:1]]) for c in codes]     # session 0 <-> row 3
    with gen.streaming(B):
        gen.set_session_adapter(3, 2); gen.set_session_adapter(0, 0); gen.set_session_adapter(1, None); gen.set_session_adapter(2, 1)
        second = run_taps(gen, moved, device)
    same_rows(first, second, [0], [3], "session 0 on slot 0 / in row 3 on the last slot")
    same_rows(first, second, [3], [0], "session 3 on the last slot / in row 0 on slot 0")


def check_all_rows_without_adapter_equal_plain(device, lib, B, steps=3, seed=52):
    """An adapter handle with every row at -1 against a plain handle under the knobs that select the same unfused launch list."""
    cfg = tiny_lm_config()
    lm, sd = adapter_model(device, lib, cfg, B, seed)
    with env(**UNFUSED):
        plain = LMModel(sd, cfg, device=device, max_batch=B, lib=lib)
    codes = rand_codes(cfg, B, steps, seed)
    kw = dict(use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=5, support_out_of_sync=True)
    ga, gp = LMGen(lm, **kw), LMGen(plain, **kw)
    with ga.streaming(B):
        a = run_taps(ga, codes, device)
        la = ga.launch_list()
    with gp.streaming(B):
        p = run_taps(gp, codes, device)
        lp = gp.launch_list()
    same_rows(a, p, slice(None), slice(None), f"adapter handle at -1 against a plain handle, B={B}")
    assert [s for s, _ in la if not s.endswith(".lora")] == [s for s, _ in lp], "the adapter handle's launch list minus its shrink launches is the unfused plain list"
    assert sum(s.endswith(".lora") for s, _ in la) == sum("gemm" in k for _, k in lp), "one shrink launch per linear"
    return la


def check_unused_slot_changes_nothing(device, lib, B=3, steps=3, seed=53):
    cfg = tiny_lm_config()
    lm, sd = adapter_model(device, lib, cfg, B, seed, loaded=(0,))
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    codes = rand_codes(cfg, B, steps, seed)
    with gen.streaming(B):
        gen.set_session_adapter(1, 0)
        a = run_taps(gen, codes, device)
    lm.load_adapter(2, random_adapter(sd, 32, 77, 4.0, 4.0), scaling=2.0)
    with gen.streaming(B):
        gen.set_session_adapter(1, 0)
        b = run_taps(gen, codes, device)
    same_rows(a, b, slice(None), slice(None), "an adapter loaded into a slot no row uses")


def check_guidance_twins_take_the_adapter(device, lib, steps=2, seed=54):
    """Under guidance both model rows of a session take its adapter.  cfg_coef = 0 makes the audio logits the UNCONDITIONED row's
    alone (null + (cond - null) * 0) and cfg_is_no_text keeps the CONDITIONED row's text logits: with every run teacher-forced on
    the same tokens, a session on an adapter must differ from its base run in both, its neighbour in neither, and the session
    gives the same numbers in either row."""
    cfg = tiny_lm_config()
    B = 2
    lm, sd = adapter_model(device, lib, cfg, 2 * B, seed)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=0.0, cfg_is_no_text=True)
    codes = rand_codes(cfg, B, steps, seed)
    with gen.streaming(B):
        base = run_taps(gen, codes, device)
    forced = [np.concatenate([tl.argmax(1, keepdim=True).numpy(), al.argmax(2).numpy()], 1) for _, tl, al in base]
    with gen.streaming(B):
        base = run_taps(gen, codes, device, forced)
    with gen.streaming(B):
        gen.set_session_adapter(0, 0)
        a = run_taps(gen, codes, device, forced)
    with gen.streaming(B):
        gen.set_session_adapter(1, 0)
        b = run_taps(gen, [c.flip(0) for c in codes], device, [f[::-1].copy() for f in forced])
    same_rows(a, base, [1], [1], "the session without an adapter, guided")
    same_rows(a, b, [0], [1], "a guided session on slot 0, in row 0 and in row 1")
    for s in range(steps):
        assert not torch.equal(a[s][1][0], base[s][1][0]), f"step {s}: the conditioned row did not take the adapter"
        assert not torch.equal(a[s][2][0], base[s][2][0]), f"step {s}: the unconditioned row (the guidance twin) did not take the adapter"


# ---- e. repeat streams ---------------------------------------------------------------------------------------------------------------------------------
def check_repeat_streams(device, lib, B, repeats=2, steps=3, seed=55):
    """Two streams fed the same frames on one adapter handle with mixed slots: bit-identical."""
    cfg = tiny_lm_config()
    lm, sd = adapter_model(device, lib, cfg, B, seed)
    gen = LMGen(lm, use_sampling=True, temp=0.9, temp_text=0.8, top_k=20, top_k_text=10, seed=5, support_out_of_sync=True)
    codes = rand_codes(cfg, B, steps, seed)
    runs = []
    for _ in range(repeats):
        with gen.streaming(B):
            for i in range(B):
                gen.set_session_adapter(i, (i % 4) - 1 if i % 4 else None)
            runs.append(run_taps(gen, codes, device))
    for r in runs[1:]:
        same_rows(runs[0], r, slice(None), slice(None), f"repeat stream, B={B}")


# ---- f. behaviour around the state ----------------------------------------------------------------------------------------------------------------------
def check_state_behaviour(device, lib, B=3, seed=56):
    cfg = tiny_lm_config()
    lm, sd = adapter_model(device, lib, cfg, B, seed)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    codes = rand_codes(cfg, B, 4, seed)
    with gen.streaming(B):
        assert [gen.session_adapter(i) for i in range(B)] == [None] * B            # streaming_start: every row at -1
        base = run_taps(gen, codes, device)
    with gen.streaming(B):
        first = run_taps(gen, codes[:2], device)
        gen.set_session_adapter(1, 0)                                               # mid-stream: from the next step on
        snap = gen.get_streaming_state()
        rest = run_taps(gen, codes[2:], device)
        # load / unload / set while the step is captured: the program is not rebuilt
        launches, captured = gen.launch_list(), lm._lib.mmi_lm_stat(lm._handle, 1)
        if torch.device(device).type != "cpu":       # (the simulator has no graph capture: its list runs eagerly)
            assert captured != 0, "no step program is captured after four steps: the check below would compare nothing"
        lm.load_adapter(2, random_adapter(sd, 32, 31, 1.0, 1.0))
        lm.unload_adapter(2)
        gen.set_session_adapter(2, 1); gen.set_session_adapter(2, None)
        run_taps(gen, codes[:1], device)
        assert lm._lib.mmi_lm_stat(lm._handle, 1) == captured and gen.launch_list() == launches
        gen.reset_streaming(torch.tensor([False, True, False]))
        assert gen.session_adapter(1) == 0                                          # a reset leaves the slot alone
        gen.set_session_adapter(1, None); gen.set_session_adapter(2, 1)
        gen.set_streaming_state(snap)                                               # the snapshot carries the slots
        assert [gen.session_adapter(i) for i in range(B)] == [None, 0, None]
        again = run_taps(gen, codes[2:], device)
    same_rows(first, base[:2], slice(None), slice(None), "before set_session_adapter")
    same_rows(rest, base[2:], [0, 2], [0, 2], "rows that kept the base model")
    assert not torch.equal(rest[0][1][1], base[2][1][1]), "set_session_adapter mid-stream did not take effect at the next step"
    same_rows(rest, again, slice(None), slice(None), "after set_streaming_state")


# ---- g. refusals --------------------------------------------------------------------------------------------------------------------------------------
def _raises(exc, match, fn):
    try:
        fn()
    except exc as e:
        assert match in str(e), f"expected '{match}' in: {e}"
        return
    raise AssertionError(f"expected {exc.__name__} ('{match}')")


def check_refusals(device, lib):
    from moshi_amd.weights import quantize_lm_state_dict, quantize_lm_state_dict_fp8, quantize_lm_state_dict_mxfp4
    cfg = tiny_lm_config()
    sd = cached_lm_state_dict(cfg, 57)
    mk = lambda **kw: LMModel(kw.pop("sd", sd), kw.pop("cfg", cfg), device=device, max_batch=kw.pop("max_batch", 2), lib=lib, **kw)
    # enable
    for q in (quantize_lm_state_dict, quantize_lm_state_dict_fp8):
        _raises(NotImplementedError, "quantised linears", lambda: mk(sd=q(sd), adapters=(2, 32)))
    mxcfg = replace(cfg, card=72, depformer_dim_feedforward=240)
    _raises(NotImplementedError, "quantised linears", lambda: mk(sd=quantize_lm_state_dict_mxfp4(cached_lm_state_dict(mxcfg, 57)), cfg=mxcfg, adapters=(2, 32)))
    _raises(NotImplementedError, "above 64 model rows", lambda: LMModel(sd, cfg, device=device, max_rows=65, lib=lib, adapters=(2, 32)))
    xcfg = replace(cfg, cross_attention=True)
    _raises(NotImplementedError, "cross-attention", lambda: mk(sd=cached_lm_state_dict(xcfg, 57), cfg=xcfg, adapters=(2, 32)))
    hcfg = replace(cfg, extra_heads_num_heads=2, extra_heads_dim=6)
    _raises(NotImplementedError, "extra heads", lambda: mk(sd=cached_lm_state_dict(hcfg, 57), cfg=hcfg, adapters=(2, 32)))
    lrcfg = replace(cfg, depformer_weights_per_step_schedule=[0] + [1] * 7, depformer_low_rank_embeddings=16)
    _raises(NotImplementedError, "low-rank or demuxed embeddings", lambda: mk(sd=cached_lm_state_dict(lrcfg, 57), cfg=lrcfg, adapters=(2, 32)))
    dmcfg = replace(cfg, demux_second_text_stream=True)
    _raises(NotImplementedError, "low-rank or demuxed embeddings", lambda: mk(sd=cached_lm_state_dict(dmcfg, 57), cfg=dmcfg, adapters=(2, 32)))
    with env(MMI_DEP_TILE="16"):                    # the depth transformer on its own 16-row tile (17..32 rows)
        _raises(NotImplementedError, "MMI_DEP_TILE", lambda: mk(max_batch=18, adapters=(2, 32)))
    _raises(ValueError, "max_adapters must be 1..8", lambda: mk(adapters=(9, 32)))
    _raises(ValueError, "max_rank must be 32, 64, 96 or 128", lambda: mk(adapters=(2, 48)))
    plain = mk()
    _raises(RuntimeError, "no adapters", lambda: plain.load_adapter(0, {}))
    gp = LMGen(plain, use_sampling=False)
    with gp.streaming(2):
        _raises(NotImplementedError, "before streaming_start", lambda: lib.check(lib.mmi_lm_enable_adapters(plain._handle, 2, 32)))
        _raises(RuntimeError, "not enabled", lambda: gp.set_session_adapter(0, 0))
    lib.check(lib.mmi_lm_enable_adapters(plain._handle, 2, 32))                     # and (0, 0) turns them off again
    lib.check(lib.mmi_lm_enable_adapters(plain._handle, 0, 0))
    _raises(RuntimeError, "no adapters", lambda: plain.load_adapter(0, {}))
    # load
    lm = mk(adapters=(2, 32))
    good = random_adapter(sd, 32, 1)
    stem = "transformer.layers.0.gating.linear_in"
    bad = dict(good); bad["transformer.layers.0.nope.lora_A.weight"] = good[stem + ".lora_A.weight"]
    _raises(ValueError, "unexpected_keys in the lora weights", lambda: lm.load_adapter(0, bad))
    bad = dict(good); del bad[stem + ".lora_B.weight"]
    _raises(ValueError, "without", lambda: lm.load_adapter(0, bad))
    _raises(ValueError, "at most max_rank", lambda: lm.load_adapter(0, random_adapter(sd, 64, 1)))
    _raises(ValueError, "multiple of 8", lambda: lm.load_adapter(0, random_adapter(sd, 12, 1)))
    bad = dict(good); bad[stem + ".lora_A.weight"] = good[stem + ".lora_A.weight"][:, :-8].contiguous()
    _raises(ValueError, "do not fit", lambda: lm.load_adapter(0, bad))
    bad = dict(good); b = good[stem + ".lora_B.weight"].clone(); b[3, 5] = float("inf"); bad[stem + ".lora_B.weight"] = b
    _raises(ValueError, "not finite", lambda: lm.load_adapter(0, bad))
    bad = dict(good); b = good[stem + ".lora_B.weight"].clone(); b[3, 5] = 3e38; bad[stem + ".lora_B.weight"] = b      # finite, but 2 * b is not
    _raises(ValueError, "not finite", lambda: lm.load_adapter(0, bad))
    _raises(ValueError, "slot outside", lambda: lm.load_adapter(2, good))
    lm.load_adapter(0, good)
    gen = LMGen(lm, use_sampling=False)
    with gen.streaming(2):
        _raises(ValueError, "slot must be -1", lambda: gen.set_session_adapter(0, 2))
        _raises(ValueError, "session outside", lambda: gen.set_session_adapter(2, 0))
        gen.set_session_adapter(1, 0)
        _raises(RuntimeError, "a live session runs on this slot", lambda: lm.load_adapter(0, good))
        _raises(RuntimeError, "a live session runs on this slot", lambda: lm.unload_adapter(0))
        lm.load_adapter(1, good)                                                    # another slot: allowed while streaming
        gen.set_session_adapter(1, None)
        lm.unload_adapter(0)
        _raises(NotImplementedError, "plain and the split-K path",
                lambda: lm.debug_linear_lora("depformer.layers.0.self_attn.in_projs.0.weight", torch.zeros(1, cfg.depformer_dim), [0], path="norm_fused"))


# ---- h. plain handles do not notice ----------------------------------------------------------------------------------------------------------------------
def check_other_classes_do_not_notice(device, lib, B=3, steps=2, seed=58):
    from moshi_amd.weights import quantize_lm_state_dict, quantize_lm_state_dict_fp8, quantize_lm_state_dict_mxfp4
    cfg = replace(tiny_lm_config(), card=72, depformer_dim_feedforward=240)           # (MXFP4 needs in_features % 32 == 0)
    sd = cached_lm_state_dict(cfg, seed)
    codes = rand_codes(cfg, B, steps, seed)

    def run(q):
        state = {"bf16": lambda s: s, "int8": quantize_lm_state_dict, "fp8": quantize_lm_state_dict_fp8, "mxfp4": quantize_lm_state_dict_mxfp4}[q](sd)
        gen = LMGen(LMModel(state, cfg, device=device, max_batch=B, lib=lib), use_sampling=False, support_out_of_sync=True)
        with gen.streaming(B):
            out = run_taps(gen, codes, device)
            return out, gen.launch_list()
    before = {q: run(q) for q in ("bf16", "int8", "fp8", "mxfp4")}
    lm = LMModel(sd, cfg, device=device, max_batch=B, lib=lib, adapters=(2, 32))
    lm.load_adapter(0, random_adapter(sd, 32, 3, 1.0, 1.0))
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    with gen.streaming(B):
        gen.set_session_adapter(0, 0)
        run_taps(gen, codes, device)
    for q, (out, ll) in before.items():
        out2, ll2 = run(q)
        assert ll == ll2, f"{q}: launch list changed"
        assert not any(s.endswith(".lora") for s, _ in ll)
        same_rows(out, out2, slice(None), slice(None), f"{q} handle before / after an adapter handle ran")


# ---- the batcher --------------------------------------------------------------------------------------------------------------------------------------------
def check_batcher_open_close(device, lib):
    from moshi_amd import MimiModel, SessionBatcher, tiny_mimi_config
    from moshi_amd.weights import random_mimi_state_dict
    cfg = tiny_lm_config()
    lm, sd = adapter_model(device, lib, cfg, 2, 59)
    mcfg = replace(tiny_mimi_config(), q_bins=cfg.card, q_n_q=cfg.dep_q)
    mimi = MimiModel(random_mimi_state_dict(mcfg, seed=7), mcfg, device=device, max_batch=2, num_codebooks=cfg.dep_q, lib=lib)
    slot_of = lambda r: int(lib.mmi_lm_row_adapter(lm._handle, r))
    with SessionBatcher(mimi, lm, slots=2, use_sampling=False) as bt:
        _raises(ValueError, "slot must be -1", lambda: bt.open(adapter=3))
        a = bt.open(adapter=1)
        b = bt.open()
        pcm = np.zeros(bt.frame_size, np.float32)
        bt.push(a, pcm); bt.push(b, pcm)
        bt.step()
        assert (slot_of(0), slot_of(1)) == (1, -1)
        bt.close(a)
        bt.step()
        assert slot_of(0) == -1                                                     # close returns the row to -1
        c = bt.open()                                                               # a reopened channel starts at -1
        bt.push(c, pcm)
        bt.step()
        assert slot_of(0) == -1


def smoke_adapters(device, lib=None):
    return check_golden_mixed_slots(device, lib)
