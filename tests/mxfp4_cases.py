"""Cases for OCP MXFP4 linears (`weight` uint8 E2M1 code pairs + `weight_scale_e8m0`; k_pack_w_fp4, k_gemm_xp / k_gemm_xp_norm
WQ = 4, mmi_fp4.h), shared by the simulator tests (tests/test_mxfp4_sim.py) and the GPU tests (tests/test_z_mxfp4_gpu.py).

The conversion is exact (one mantissa bit times a power of two is a bf16 value), so the yardstick throughout is the bf16
arithmetic on `dequantize_lm_state_dict_mxfp4(sd)`: single weights bit for bit (one-hot rows), whole linears on sums that are
exact in fp32 in any order, the network against the bf16 oracle on the dequantised state dict under the bf16 engine's own gates.

Shapes: every in_features must be a multiple of 32 (the MX block), so the depth transformer's hidden size is 160 here
(`depformer_dim_feedforward=240`) instead of the tiny config's 176 - 176 is the refusal case.  A gated linear's N is its
linear_out's K and therefore a multiple of 32 as well: a gated N "off the tile" cannot exist in this format; the odd
out_features kept are card = 72 (a last n-tile of 8 features) and N = 160 (five 32-row tiles, ten 16-row tiles)."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import torch

from moshi_amd.config import tiny_lm_config, tiny_stt_config
from moshi_amd.lm import LMGen, LMModel
from moshi_amd.weights import (MXFP4_SCALE_SUFFIX, dequantize_lm_state_dict_mxfp4, dequantize_mxfp4, is_lm_linear_weight,
                               quantize_lm_state_dict_mxfp4, quantize_mxfp4)
from oracle.lm_oracle import LMOracle, bf16r, silu
from tests import lm_cases as lc
from tests.lm_cases import _bf16_bits, _dyadic_rows, cached_lm_state_dict
from tests.many_rows_cases import env, linear_sites

SFX = MXFP4_SCALE_SUFFIX


def mx_config():
    return replace(tiny_lm_config(), card=72, depformer_dim_feedforward=240)


def pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """[N, K] codes 0..15 -> [N, K / 2] bytes, element 2i in the low nibble."""
    codes = codes.to(torch.uint8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


# ---- 1. the quantiser (CPU) -----------------------------------------------------------------------------------------------------------------
def check_quantiser_crafted_blocks():
    def q(block):
        v = torch.zeros(1, 32)
        v[0, :len(block)] = torch.tensor(block, dtype=torch.float32)
        c, s = quantize_mxfp4(v)
        codes = torch.stack([c & 15, c >> 4], 2).reshape(-1)[:len(block)].tolist()
        return codes, int(s[0, 0])
    # ties go to the even code: absmax 4 -> scale 2^0; the midpoints 0.25 .75 1.25 1.75 2.5 3.5 (5 needs absmax >= 5: below)
    codes, s = q([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25, -0.75, -2.5])
    assert s == 127 and codes == [6, 0, 2, 2, 4, 4, 6, 8, 8 | 2, 8 | 4], (codes, s)
    codes, s = q([6.0, 5.0, -5.0, 4.99, 5.01])
    assert s == 127 and codes == [7, 6, 8 | 6, 6, 7], (codes, s)
    # saturation: absmax 7.5 has floor(log2) = 2 -> scale 2^0, 7.5 / 1 is beyond the largest value
    codes, s = q([7.5, -7.9, 7.0, 1.0])
    assert s == 127 and codes == [7, 15, 7, 2], (codes, s)
    # an all-zero block
    c, sc = quantize_mxfp4(torch.zeros(2, 64))
    assert int(c.max()) == 0 and sc.tolist() == [[127, 127], [127, 127]]
    # absmax an exact power of two: 2^k -> scale 2^(k - 2), the element is 4.0 (code 6)
    for k in (-9, 0, 5):
        codes, s = q([2.0 ** k, -(2.0 ** k) / 8, 2.0 ** k * 0.75])
        assert s == 127 + k - 2 and codes == [6, 8 | 1, 5], (k, codes, s)
    # a non-multiple of the block is refused
    try:
        quantize_mxfp4(torch.zeros(4, 176))
    except ValueError as e:
        assert "multiple of 32" in str(e)
    else:
        raise AssertionError("in_features = 176 was quantised")


def check_quantise_dequantise_quantise():
    cfg = mx_config()
    sd = cached_lm_state_dict(cfg, 5)
    q1 = quantize_lm_state_dict_mxfp4(sd)
    lin = [k for k in sd if is_lm_linear_weight(k)]
    assert lin and all(q1[k].dtype == torch.uint8 and q1[k + SFX].dtype == torch.uint8 for k in lin)
    assert all(tuple(q1[k].shape) == (sd[k].shape[0], sd[k].shape[1] // 2) and tuple(q1[k + SFX].shape) == (sd[k].shape[0], sd[k].shape[1] // 32)
               for k in lin)
    assert all(torch.equal(q1[k], sd[k]) for k in sd if k not in lin)             # embeddings and norms untouched
    dq = dequantize_lm_state_dict_mxfp4(q1)
    assert set(dq) == set(sd) and all(dq[k].dtype == torch.bfloat16 for k in lin)
    q2 = quantize_lm_state_dict_mxfp4(dq)
    assert set(q1) == set(q2) and all(torch.equal(q1[k], q2[k]) for k in q1), "quantise(dequantise(q)) != q"
    assert all(torch.equal(v, quantize_lm_state_dict_mxfp4(q1)[k]) for k, v in q1.items())      # an MXFP4 state dict is kept as is
    # exact: the float64 value of every code under its scale is the bf16 that came out
    k = lin[0]
    c = torch.stack([q1[k] & 15, q1[k] >> 4], 2).reshape(sd[k].shape).numpy()
    mag = np.array([0, .5, 1, 1.5, 2, 3, 4, 6], np.float64)[c & 7] * np.where(c & 8, -1.0, 1.0)
    val = mag * np.repeat(2.0 ** (q1[k + SFX].numpy().astype(np.float64) - 127), 32, axis=1)
    assert np.array_equal(val, dq[k].double().numpy())
    # the quantisation error of a block is at most half a step of its top binade: absmax / 4 (saturation included: 8 -> 6)
    err = (dq[k].float() - sd[k].float()).abs().reshape(sd[k].shape[0], -1, 32).amax(2)
    assert bool((err <= sd[k].float().abs().reshape(sd[k].shape[0], -1, 32).amax(2) / 4).all())


def greedy_tokens(lm, steps=3, B=2):
    cfg = lm.config
    gen = LMGen(lm, use_sampling=False)
    rng = np.random.default_rng(3)
    out = []
    with gen.streaming(B):
        for _ in range(steps):
            codes = torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(lm.device)
            t = gen.step(codes)
            out.append(None if t is None else t.cpu().numpy())
    return out


def check_exporter_round_trip(lib, tmp_path, device="cpu"):
    import json
    from safetensors.torch import load_file, save_file
    from moshi_amd import loaders
    from moshi_amd.weights import random_lm_state_dict
    cfg = mx_config()
    sd = random_lm_state_dict(cfg, seed=9)
    save_file(sd, str(tmp_path / "model.safetensors"))
    info = loaders.export_quantized(tmp_path / "model.safetensors", tmp_path / "model.mxfp4.safetensors", "mxfp4", cfg.reference_kwargs())
    q = load_file(str(tmp_path / "model.mxfp4.safetensors"))
    want = quantize_lm_state_dict_mxfp4(sd)
    assert set(q) == set(want) and all(torch.equal(q[k], want[k]) for k in q)
    assert info["quantized"] == sum(is_lm_linear_weight(k) for k in sd) > 0
    (tmp_path / "config.json").write_text(json.dumps({**cfg.reference_kwargs(), "moshi_name": "model.mxfp4.safetensors",
                                                      "mimi_name": "mimi.safetensors", "tokenizer_name": "tokenizer.model"}))
    lm = loaders.CheckpointInfo.from_local(tmp_path).get_moshi(device=device, max_batch=2, lib=lib)
    assert lm.quantized
    ref = LMModel(sd, cfg, device=device, max_batch=2, lib=lib, quantize="mxfp4")
    a, b = greedy_tokens(lm), greedy_tokens(ref)
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))
    lm2 = loaders.get_moshi_lm(tmp_path / "model.safetensors", cfg.reference_kwargs(), device=device, max_batch=2, lib=lib, quantize="mxfp4")
    assert lm2.quantized


# ---- 2. conversion and layout: one-hot rows ------------------------------------------------------------------------------------------------
ONE_HOT_KEYS = ("transformer.layers.0.self_attn.out_projs.0.weight",       # K = 128: one (16-row tile) or two (32-row tile) entries
                "transformer.layers.1.gating.linear_out.weight")           # K = 352: a padded last entry at either tile


def all_codes_weight(N, K):
    """Every block holds all 16 codes (twice), in an order that differs from row to row and block to block; the scale bytes
    are spread over 100..150."""
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    codes = (k + 5 * n + 3 * (k // 32)) % 16
    scales = 100 + (7 * np.arange(N)[:, None] + 13 * np.arange(K // 32)[None, :]) % 51
    return pack_codes(torch.from_numpy(codes)), torch.from_numpy(scales.astype(np.uint8))


def one_hot_state_dict(cfg, seed=11):
    sd = quantize_lm_state_dict_mxfp4(cached_lm_state_dict(cfg, seed))
    for key in ONE_HOT_KEYS:
        N, K = sd[key].shape[0], sd[key].shape[1] * 2
        sd[key], sd[key + SFX] = all_codes_weight(N, K)
    return sd


def check_one_hot_columns(device, lib, max_batch):
    """x = e_k through the GEMM: output row b is column k_b of the dequantised weight - a bf16 times 1.0 summed with zeros is
    exact, so the comparison is on values bit for bit (a -0 weight comes out as the +0 sum: compared as equal numbers).  Holds
    the hardware conversion (nibble order, byte select, sign, every code, 51 scales) and k_pack_w_fp4's layout (codes and scale
    bytes) to the restatement."""
    cfg = mx_config()
    sd = one_hot_state_dict(cfg)
    lm = LMModel(sd, cfg, device=device, max_batch=max_batch, lib=lib)
    span = 128 if max_batch <= 16 else 64                     # features of one weight entry: four k-steps
    for key in ONE_HOT_KEYS:
        w = dequantize_mxfp4(sd[key], sd[key + SFX]).float().numpy()
        assert len(np.unique(sd[key + SFX].numpy())) == 51
        K = w.shape[1]
        whole = range(span, 2 * span) if K >= 2 * span else range(0, min(K, span))       # every k of one whole entry
        ks = sorted(set(whole) | {0, 1, K - 2, K - 1} | set(range(0, min(K, 2 * span), 7)))
        for i in range(0, len(ks), max_batch):
            chunk = ks[i:i + max_batch]
            x = np.zeros((len(chunk), K), np.float32)
            x[np.arange(len(chunk)), chunk] = 1.0
            out = lm.debug_linear(key, torch.from_numpy(x), path="plain")["out"].float().cpu().numpy()
            ref = w[:, chunk].T
            bad = np.argwhere(_bf16_bits(out + 0.0) != _bf16_bits(ref + 0.0))
            assert not len(bad), f"{key} max_batch={max_batch}: {len(bad)} weights differ, first k={chunk[bad[0][0]]} n={bad[0][1]}: " \
                                 f"{out[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


# ---- 3. every linear family on exact sums --------------------------------------------------------------------------------------------------
# The rule of many_rows_cases.check_linears_exact for this format.  Weights are built directly as codes under scale bytes
# {118, 119, 120}: every weight is a multiple of 2^-10 of magnitude <= 6 * 2^-7 < 2^-4.  Rows are lm_cases._dyadic_rows
# (+-2^-2..2^1): every product is a multiple of 2^-12, a row of K <= 352 sums to at most 352 * 2 * 6 * 2^-7 = 33 = 135168 units
# < 2^24, so the float64 sum of the dequantised operands is exact in fp32 in ANY order.  Plain linears: bf16 output IDENTICAL;
# gated: >= 99.9 % identical and everywhere within one bf16 step (2^-7 relative) - the two figures of that file.
# norm_fused (the depth transformer's k_gemm_xp_norm): the same rule needs the NORMALISED row on a grid.  Rows of one magnitude
# 2^j, j in {-1, 0, 1}, random signs: mean(x^2) = 4^j and fp32(4^j + 1e-8) = 4^j (1e-8 is under half an ulp of 0.25), rsqrt = 2^-j
# exactly; alpha is set to powers of two 2^-2..2^1: y = x * (alpha * 2^-j) = +-alpha, a bf16 value, and the sum over y * W is
# exact as above.
EXACT_ROWS = {16: (1, 16), 32: (1, 16, 17), 64: (1, 16, 17, 33, 64)}
SCALE_BYTES = (118, 119, 120)


def exact_state_dict(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    sd = dict(cached_lm_state_dict(cfg, seed))
    for key in [k for k in sd if is_lm_linear_weight(k)]:
        N, K = sd[key].shape
        sd[key] = pack_codes(torch.randint(0, 16, (N, K), generator=g))
        sd[key + SFX] = torch.tensor(SCALE_BYTES, dtype=torch.uint8)[torch.randint(0, 3, (N, K // 32), generator=g)]
    for key in [k for k in sd if k.startswith("depformer.") and ".norm" in k and k.endswith(".alpha")]:
        sd[key] = (2.0 ** torch.randint(-2, 2, sd[key].shape, generator=g).float()).to(torch.bfloat16)
    return sd


def _reference(x64, w64, gated):
    # exact in any order: every partial sum of a row's products, in units of 2^-12, stays below 2^24 - asserted on an upper bound
    # of sum_k |x_bk| |w_nk| (each column's largest |w|), then on the float64 sum itself
    assert (np.abs(x64) @ np.abs(w64).max(0)).max() < 2.0 ** 12, "the sum of |products| leaves the range in which fp32 is exact in any order"
    h64 = x64 @ w64.T
    assert np.abs(h64).max() < 2.0 ** 12
    h = bf16r(h64.astype(np.float32))
    if gated:
        H = h.shape[1] // 2
        return bf16r(bf16r(silu(h[:, :H])) * h[:, H:])
    return h


def _compare(out, ref, gated, name):
    same = _bf16_bits(out) == _bf16_bits(ref)
    if gated:
        ulp = np.abs(out - ref) <= np.maximum(np.abs(ref), 1e-30) * 2.0 ** -7
        assert same.mean() >= 0.999 and ulp.all(), f"{name}: gated output {same.mean():.5f} identical, worst {np.abs(out - ref).max()}"
    else:
        assert same.all(), f"{name}: {int((~same).sum())} of {same.size} bf16 outputs differ (first at {np.argwhere(~same)[0]})"


def check_linears_exact(device, lib, max_batch, ksplit=None, seed=31):
    cfg = mx_config()
    sd = exact_state_dict(cfg, seed)
    dq = dequantize_lm_state_dict_mxfp4(sd)
    with env(**({"MMI_GEMM_KSPLIT": ksplit} if ksplit else {})):
        lm = LMModel(sd, cfg, device=device, max_batch=max_batch, lib=lib)
    rng = np.random.default_rng(seed)
    k_last = cfg.dep_q - 1
    sites = [(key, paths, None) for key, paths in linear_sites(cfg)]
    sites += [(f"depformer.layers.0.self_attn.in_projs.{k_last}.weight", ["norm_fused"], "depformer.layers.0.norm1.alpha"),
              ("depformer.layers.1.gating.2.linear_in.weight", ["norm_fused"], "depformer.layers.1.norm2.alpha")]
    checked = split = 0
    for key, paths, alpha_key in sites:
        w = dq[key].double().numpy()
        gated = "linear_in" in key
        for path in paths:
            for B in EXACT_ROWS[max_batch]:
                K = w.shape[1]
                if path == "norm_fused":
                    x = (2.0 ** rng.integers(-1, 2, (B, 1)) * rng.choice([-1.0, 1.0], (B, K))).astype(np.float32)
                    y = np.sign(x).astype(np.float64) * dq[alpha_key].double().numpy().reshape(1, K)
                else:
                    x = _dyadic_rows(rng, B, K)
                    y = x.astype(np.float64)
                try:
                    out = lm.debug_linear(key, torch.from_numpy(x), path=path, alpha_name=alpha_key)["out"].float().cpu().numpy()
                except NotImplementedError as e:
                    if path == "splitk" and "does not split" in str(e):      # tiny shapes are not split over K unless forced
                        continue
                    raise
                _compare(out, _reference(y, w, gated), gated, f"{key} [{path}] rows={B} max_batch={max_batch} ksplit={ksplit}")
                checked += 1
                split += path == "splitk"
    if ksplit and ksplit > 1:       # a linear is split where it has at least `ksplit` weight entries: K = 352 always has (3 at the 16-row tile)
        assert split >= len(EXACT_ROWS[max_batch]), f"MMI_GEMM_KSPLIT={ksplit}: only {split} split-K cases ran"
    return checked


# ---- 7. the 7B layer's shapes (GPU only) ---------------------------------------------------------------------------------------------------
def check_7b_layer_shapes(device, lib, seed=5):
    """in_proj (4096 -> 12288), the gated linear_in (4096 -> 2 x 11264) and the split-K linear_out (11264 -> 4096) of one 7B layer
    at 32 and 64 rows: the production wave and split-K plans.  Weights as in check_linears_exact (multiples of 2^-10, <= 6 * 2^-7);
    the rows are scaled to +-2^-2..2^-1 so that a sum over 11264 features stays at most 11264 * 2^-1 * 6 * 2^-7 = 264 = 1081344
    units of 2^-12 < 2^24 (asserted on the float64 sum)."""
    from moshi_amd.config import LMConfig
    cfg = replace(mx_config(), dim=4096, num_heads=32, num_layers=1, hidden_scale=4.125, context=8, text_card=64)
    assert cfg.ffn_hidden == 11264 and isinstance(cfg, LMConfig)
    sd = exact_state_dict(cfg, seed)
    lm = LMModel(sd, cfg, device=device, max_batch=64, lib=lib)
    rng = np.random.default_rng(seed)
    for key, path in (("transformer.layers.0.self_attn.in_projs.0.weight", "plain"), ("transformer.layers.0.gating.linear_in.weight", "plain"),
                      ("transformer.layers.0.gating.linear_out.weight", "splitk")):
        w = dequantize_mxfp4(sd[key], sd[key + SFX]).double().numpy()
        K = w.shape[1]
        x = (2.0 ** rng.integers(-2, 0, (64, K)) * rng.choice([-1.0, 1.0], (64, K))).astype(np.float32)
        ref = _reference(x.astype(np.float64), w, "linear_in" in key)               # once: the 32-row case reads its first rows
        for B in (32, 64):
            out = lm.debug_linear(key, torch.from_numpy(x[:B]), path=path)["out"].float().cpu().numpy()
            _compare(out, ref[:B], "linear_in" in key, f"7B {key} [{path}] rows={B}")


# ---- 4. the network against the bf16 oracle on the dequantised weights ----------------------------------------------------------------------
def check_network_vs_oracle(device, lib, kind, B, S=2, seed=None):
    """LMGen on the MXFP4 state dict against LMOracle on its dequantisation, under the gates lm_cases holds the bf16 engine to
    against its oracle (logits_close / near_tie: LOGIT_MAX_REL and the mean gate, imported): the claim is "a correct engine on
    these weights".  Masks and a partial reset as in lm_cases.oracle_vs_engine."""
    cfg = mx_config() if kind == "moshi" else tiny_stt_config()
    seed = 1700 + B if seed is None else seed
    sd = quantize_lm_state_dict_mxfp4(cached_lm_state_dict(cfg, seed))
    gen = LMGen(LMModel(sd, cfg, device=device, max_batch=B, lib=lib), use_sampling=False, support_out_of_sync=True)
    assert gen.lm_model.quantized
    orc = LMOracle(dequantize_lm_state_dict_mxfp4(sd), cfg)
    orc.streaming(B)
    rng = np.random.default_rng(seed)
    with gen.streaming(B):
        for s in range(S):
            mask = rng.random(B) > 0.3
            mask[0] = True
            if s == S // 2:
                r = np.zeros(B, bool); r[B - 1] = True
                orc.reset_streaming(r); gen.reset_streaming(torch.from_numpy(r).to(device))
                mask[B - 1] = True
            orc.set_exec_mask(mask); gen.set_exec_mask(torch.from_numpy(mask).to(device))
            codes = rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))
            oo, (otl, oal, ott, oat) = orc.step(codes, use_sampling=False, support_out_of_sync=True)
            forced = np.concatenate([ott[:, None], oat], 1)
            out, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device), forced_tokens=torch.from_numpy(forced).to(device))
            out, tl, al = out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy()
            for b in np.flatnonzero(mask):
                assert np.array_equal(out[b], oo[b]), f"step {s} row {b}: ring output differs"
                assert lc.logits_close(tl[b], otl[b]), f"step {s} row {b}: text logits {np.abs(tl[b] - otl[b]).max()}"
                for k in range(cfg.dep_q):
                    assert lc.logits_close(al[b, k], oal[b, k]), f"step {s} row {b} cb {k}: {np.abs(al[b, k] - oal[b, k]).max()}"
                    a_e, a_o = int(al[b, k].argmax()), int(oat[b, k])
                    assert a_e == a_o or lc.near_tie(oal[b, k], a_e, a_o)
        kernels = {k for _, k in gen.launch_list()}
    assert "k_gemm_xp" in kernels, kernels
    assert not kernels & {"k_gemm_xlds", "k_gemm_xp_once", "k_gemm_rows", "k_dep_attn_out_proj"}, kernels
    if cfg.dep_q:
        assert "k_gemm_xp_norm" in kernels, kernels       # the depth transformer's norms stay inside their GEMMs
    return kernels


# ---- 5. the same stream twice on one handle ------------------------------------------------------------------------------------------------
def check_repeat_streams(device, lib, B, steps=3, repeats=1, seed=77):
    cfg = mx_config()
    sd = quantize_lm_state_dict_mxfp4(cached_lm_state_dict(cfg, seed + B))
    gen = LMGen(LMModel(sd, cfg, device=device, max_batch=B, lib=lib), use_sampling=False, support_out_of_sync=True)
    gen.lm_model.enable_hidden_taps()
    rng = np.random.default_rng(seed)
    plan = []
    for s in range(steps):
        mask = rng.random(B) > 0.3
        mask[0] = True
        reset = None
        if s == 1 and B > 1:
            reset = np.zeros(B, bool); reset[B - 1] = True
        plan.append((mask, reset, rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))))

    def run():
        out = []
        with gen.streaming(B):
            for mask, reset, codes in plan:
                if reset is not None:
                    gen.reset_streaming(torch.from_numpy(reset).to(device))
                gen.set_exec_mask(torch.from_numpy(mask).to(device))
                o, tl, al = gen.step_with_taps(torch.from_numpy(codes).to(device))
                out.append((o.cpu(), tl.cpu(), al.cpu(), gen.hidden_taps().cpu()))
        return out
    first = run()
    for r in range(repeats):
        for s, (a, b) in enumerate(zip(first, run())):
            m = torch.from_numpy(plan[s][0])
            for name, x, y in zip(("tokens", "text logits", "audio logits"), a[:3], b[:3]):
                assert torch.equal(x[m], y[m]), f"repeat {r} step {s}: {name} differ between two streams fed the same frames"
            for w in (0, 1):
                assert torch.equal(a[3][w][m], b[3][w][m]), f"repeat {r} step {s}: the residual stream (tap {w}) differs"


# ---- 6. refusals; the other weight classes do not notice -----------------------------------------------------------------------------------
def check_refusals(device, lib):
    import pytest
    cfg = mx_config()
    good = quantize_lm_state_dict_mxfp4(cached_lm_state_dict(cfg, 21))
    key = "transformer.layers.1.self_attn.out_projs.0.weight"

    def load(sd, c=cfg, **kw):
        return LMModel(sd, c, device=device, lib=lib, **({"max_batch": 4} if not kw else kw))
    # in_features off the MX block: the repository's tiny config has K = 176 in the depth transformer's linear_out
    tiny = tiny_lm_config()
    with pytest.raises(ValueError, match="linear_out.weight.*multiple of 32"):
        quantize_lm_state_dict_mxfp4(cached_lm_state_dict(tiny, 21))
    crafted = quantize_lm_state_dict_mxfp4({k: v for k, v in cached_lm_state_dict(tiny, 21).items() if not ("depformer" in k and "linear_out" in k)})
    for k, v in cached_lm_state_dict(tiny, 21).items():
        if "depformer" in k and "linear_out" in k:
            crafted[k] = torch.zeros(v.shape[0], 88, dtype=torch.uint8)
            crafted[k + SFX] = torch.full((v.shape[0], 5), 127, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match=r"in_features to be a multiple of 32: depformer\.layers\.\d\.gating\.\d\.linear_out\.weight"):
        load(crafted, tiny)
    # the scale tensor: missing, mis-shaped
    with pytest.raises(KeyError, match="missing weight: " + key.replace(".", r"\.") + "_scale_e8m0"):
        load({k: v for k, v in good.items() if k != key + SFX})
    with pytest.raises(AssertionError, match="block scales must be e8m0 .out_features, in_features / 32.: " + key.replace(".", r"\.")):
        load({**good, key + SFX: good[key + SFX][:, :-1].contiguous()})
    with pytest.raises(AssertionError, match="block scales must be e8m0"):
        load({**good, key + SFX: good[key + SFX][:-1].contiguous()})
    # scale bytes: 255 is the E8M0 NaN; 254, 253, 0, 1 leave the range in which every weight is a normal, finite bf16
    def with_scale(b):
        s = good[key + SFX].clone()
        s[3, 1] = b
        return {**good, key + SFX: s}
    with pytest.raises(ValueError, match="scale 255 is the E8M0 NaN: " + key.replace(".", r"\.")):
        load(with_scale(255))
    for b in (254, 253, 0, 1):
        with pytest.raises(NotImplementedError, match=f"block scales must be 2..252 .*found {b}: " + key.replace(".", r"\.")):
            load(with_scale(b))
    for b in (2, 252):
        load(with_scale(b))
    # mixed widths
    bf = cached_lm_state_dict(cfg, 21)
    with pytest.raises(NotImplementedError, match="mixed bf16 / int8 / fp8 linear weights"):
        load({**{k: v for k, v in good.items() if k != key + SFX}, key: bf[key]})
    from moshi_amd.weights import quantize_lm_state_dict
    i8 = quantize_lm_state_dict(bf)
    with pytest.raises(NotImplementedError, match="mixed bf16 / int8 / fp8 linear weights"):
        load({**{k: v for k, v in good.items() if k != key + SFX}, key: i8[key], key + "_scb": i8[key + "_scb"]})
    # more than 64 model rows
    with pytest.raises(NotImplementedError, match="MXFP4 linears are not supported above 64 model rows"):
        load(good, max_rows=96)
    # cross-attention layers; low-rank / demuxed embeddings
    from moshi_amd.config import tiny_tts_config
    from moshi_amd.weights import random_lm_state_dict
    xcfg = replace(cfg, cross_attention=True)
    xsd = quantize_lm_state_dict_mxfp4(random_lm_state_dict(xcfg, seed=3))
    with pytest.raises(NotImplementedError, match="cross-attention layers"):
        load(xsd, xcfg)
    # the TTS-shaped tiny model with every in_features on the MX block: low-rank depformer embeddings and a demuxed text stream
    tcfg = replace(tiny_tts_config(), cross_attention=False, depformer_dim_feedforward=240)
    assert tcfg.depformer_low_rank_embeddings and tcfg.demux_second_text_stream
    tsd = quantize_lm_state_dict_mxfp4(random_lm_state_dict(tcfg, seed=3))
    with pytest.raises(NotImplementedError, match="low-rank or demuxed embeddings"):
        load(tsd, tcfg)
    # the C entry itself (LMModel refuses the last two before it is reached): hand-built descriptors
    from moshi_amd import _capi
    from moshi_amd.lm import _lm_cfg_ext_struct, _lm_cfg_struct
    import ctypes as C

    def create(sd, c):
        dsd = {k: v.to(device) if v.dtype == torch.uint8 else v.to(device=device, dtype=torch.bfloat16) for k, v in sd.items()}
        descs, keep = _capi.tensor_descs(dsd)
        h, ext = C.c_void_p(), _lm_cfg_ext_struct(c)
        if ext is None:
            rc = lib.mmi_lm_create(C.byref(_lm_cfg_struct(c)), descs, len(dsd), 4, C.byref(h))
        else:
            rc = lib.mmi_lm_create_ext(C.byref(_lm_cfg_struct(c)), C.byref(ext), descs, len(dsd), 4, C.byref(h))
        del keep
        assert not h.value
        return rc, lib.last_error()
    rc, msg = create(xsd, xcfg)
    assert rc == _capi.MMI_ERR_UNSUPPORTED and "cross-attention layers with quantised linears are not supported" in msg, (rc, msg)
    assert _lm_cfg_ext_struct(tcfg) is not None
    rc, msg = create(tsd, tcfg)
    assert rc == _capi.MMI_ERR_UNSUPPORTED and "quantised linears with low-rank or demuxed embeddings are not supported" in msg, (rc, msg)
    # low-rank embeddings alone, and a demuxed text stream alone
    for one in (replace(tcfg, demux_second_text_stream=False), replace(tcfg, depformer_low_rank_embeddings=None)):
        rc, msg = create(quantize_lm_state_dict_mxfp4(random_lm_state_dict(one, seed=3)), one)
        assert rc == _capi.MMI_ERR_UNSUPPORTED and "quantised linears with low-rank or demuxed embeddings are not supported" in msg, (rc, msg)


def check_other_classes_do_not_notice(device, lib, B=3):
    """A bf16, an int8 and an fp8 handle keep their launch list and their outputs when an MXFP4 handle is built (and run) next to
    them: the same seeded greedy step before and after."""
    cfg = mx_config()
    sd = cached_lm_state_dict(cfg, 41)

    def step(quantize):
        gen = LMGen(LMModel(sd, cfg, device=device, max_batch=B, lib=lib, quantize=quantize), use_sampling=False, support_out_of_sync=True)
        rng = np.random.default_rng(8)
        with gen.streaming(B):
            out = gen.step_with_taps(torch.from_numpy(rng.integers(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1))).to(device))
            return [f"{a}\t{b}" for a, b in gen.launch_list()], [t.cpu() for t in out]
    before = {q: step(q) for q in (False, True, "fp8")}
    l4, o4 = step("mxfp4")
    after = {q: step(q) for q in (False, True, "fp8")}
    for q in before:
        assert before[q][0] == after[q][0] and len(before[q][0]) > 20, f"quantize={q}: the launch list changed"
        assert all(torch.equal(x, y) for x, y in zip(before[q][1], after[q][1])), f"quantize={q}: the outputs changed"
    assert any("k_gemm_xp" in ln for ln in l4)
    assert not all(torch.equal(x, y) for x, y in zip(o4, before[False][1]))          # (4-bit weights are other weights)
