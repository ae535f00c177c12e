"""Golden vectors for `LMGen.step` on TTS-family LMs (depformer weight schedule, low-rank depformer embeddings, demuxed text
stream, dep_q above 16, no user audio stream), produced by RUNNING THE REFERENCE (build container only, with the reference's `moshi` package importable:
`PYTHONPATH=<reference>/moshi python tests/golden/make_golden_lm_tts.py`).

lm_tts.npz - bf16, seeded weights re-drawn from the stored seeds, B=2, greedy, `support_out_of_sync=True`, the exec-mask schedule
with one partial reset of lm_cfg.npz.  Scenarios (prefix):
  g_  tiny TTS shape (moshi_amd.config.tiny_tts_config): n_q = dep_q = 20, schedule [0..5] + [6] * 14, low-rank 16, demuxed text,
      cross-attention; a `cross` [2B, 4, dim] and a `sum` [2B, 1, dim] condition, cfg_coef 2 with cfg_is_no_text; an
      `on_text_hook` that overwrites the sampled text token with a muxed one `(second + 1) * (text_card + 1) + first` where
      `g_hook` >= 0 (second = -1 and second >= 0 both occur), and `depformer_replace_tokens` (`g_replace`) on the first two steps
  h_  Moshi shape (moshi_amd.config.tiny_lm_config) with schedule [0, 1, 1, ...] and low-rank 16 embeddings, no demux, no CFG
Recorded per step: the ring output, the logits every token was sampled from (after the guidance mix) and the sampled tokens (the
audio ones are absent on replaced steps: the reference skips the depformer there, `<p>_audio_valid`).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent


def run(lm_gen, cfg, codes, masks, reset_before, B, hook=None, replace=None):
    import moshi.models.lm as lm_mod
    S = codes.shape[0]
    out = {"tokens": [], "text_logits": [], "audio_logits": [], "text_tok": [], "audio_tok": [], "audio_valid": []}
    rec = []
    orig = lm_mod.sample_token

    def sample_token(logits, *a, **k):
        tok = orig(logits, *a, **k)
        rec.append((logits.float().numpy().reshape(logits.shape[0], -1).copy(), tok.numpy().reshape(-1).copy()))
        return tok
    step = {"s": 0}
    if hook is not None:
        def on_text_hook(tok):
            h = torch.from_numpy(hook[step["s"]])
            tok.copy_(torch.where(h >= 0, h, tok))
        lm_gen.on_text_hook = on_text_hook
    lm_mod.sample_token = sample_token
    try:
        with torch.no_grad(), lm_gen.streaming(B):
            for s in range(S):
                step["s"] = s
                rec.clear()
                if s in reset_before:
                    lm_gen.reset_streaming(torch.from_numpy(reset_before[s]))
                lm_gen.set_exec_mask(torch.from_numpy(masks[s]))
                rep = None
                if replace is not None and s < replace.shape[0]:
                    rep = torch.from_numpy(replace[s])[:, :, None]
                o = lm_gen.step(torch.from_numpy(codes[s]), depformer_replace_tokens=rep)
                out["tokens"].append(o.numpy().copy())
                out["text_logits"].append(rec[0][0]); out["text_tok"].append(rec[0][1])
                if len(rec) > 1:
                    out["audio_logits"].append(np.stack([r[0] for r in rec[1:]], 1))
                    out["audio_tok"].append(np.stack([r[1] for r in rec[1:]], 1))
                    out["audio_valid"].append(True)
                else:
                    out["audio_logits"].append(np.zeros((B, cfg.dep_q, cfg.card), np.float32))
                    out["audio_tok"].append(np.asarray(replace[s]))
                    out["audio_valid"].append(False)
    finally:
        lm_mod.sample_token = orig
    return {k: np.stack(v) for k, v in out.items()}


def main():
    from moshi.conditioners.base import ConditionFuser, ConditionType
    from moshi.models.lm import LMGen, LMModel
    from moshi_amd.config import tiny_lm_config, tiny_tts_config
    from moshi_amd.weights import random_lm_state_dict
    B, S = 2, 6
    masks = np.ones((S, B), bool)
    masks[2, 1] = False
    reset_before = {4: np.array([True, False])}
    common = dict(use_sampling=False, support_out_of_sync=True)

    def model(cfg, sd, fuser=None):
        lm = LMModel(**cfg.reference_kwargs(), fuser=fuser, device="cpu", dtype=torch.bfloat16)
        lm.load_state_dict(dict(sd), strict=True)
        return lm.eval()

    def ct(t):
        return ConditionType(t, torch.ones(t.shape[:2], dtype=torch.bool))

    # ---- g: TTS shape
    cfg = tiny_tts_config()
    seed_g = 61
    sd = random_lm_state_dict(cfg, seed=seed_g)
    g = torch.Generator().manual_seed(19)
    codes_g = np.zeros((S, B, 0, 1), np.int64)
    cross_g = (0.7 * torch.randn(2 * B, 4, cfg.dim, generator=g)).to(torch.bfloat16)
    sum_g = (0.5 * torch.randn(2 * B, 1, cfg.dim, generator=g)).to(torch.bfloat16)
    N = cfg.text_card + 1
    first = torch.randint(0, N, (S, B), generator=g)
    second = torch.randint(-1, cfg.text_card, (S, B), generator=g)
    second[0, 0], second[1, 1], second[3, 0] = -1, 5, 17           # both branches on record whatever the draw
    hook = ((second + 1) * N + first).numpy()
    hook[5, 1] = -1                                                 # < 0: the sampled token stays
    replace = torch.randint(0, cfg.card, (2, B, cfg.dep_q), generator=g).numpy()
    fuser = ConditionFuser({"sum": ["s"], "cross": ["x"]})
    gen = LMGen(model(cfg, sd, fuser), cfg_coef=2.0, cfg_is_no_text=True, condition_tensors={"s": ct(sum_g), "x": ct(cross_g)}, **common)
    out = {"g_seed": np.array([seed_g]), "g_codes": codes_g, "masks": masks, "reset_step": np.array([4]), "reset_mask": reset_before[4],
           "g_cross": cross_g.float().numpy(), "g_sum": sum_g.float().numpy(), "g_hook": hook, "g_replace": replace}
    out.update({f"g_{k}": v for k, v in run(gen, cfg, codes_g, masks, reset_before, B, hook=hook, replace=replace).items()})

    # ---- h: Moshi shape, schedule + low rank
    from dataclasses import replace as dc_replace
    hcfg = dc_replace(tiny_lm_config(), depformer_weights_per_step_schedule=[0] + [1] * 7, depformer_low_rank_embeddings=16)
    seed_h = 67
    hsd = random_lm_state_dict(hcfg, seed=seed_h)
    codes_h = torch.randint(0, hcfg.card, (S, B, hcfg.n_q - hcfg.dep_q, 1), generator=g).numpy()
    out.update({"h_seed": np.array([seed_h]), "h_codes": codes_h})
    out.update({f"h_{k}": v for k, v in run(LMGen(model(hcfg, hsd), **common), hcfg, codes_h, masks, reset_before, B).items()})
    np.savez_compressed(HERE / "lm_tts.npz", **out)
    print("lm_tts.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent.parent))
    main()
