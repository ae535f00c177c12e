"""Golden vectors for `LMGen.step` with unmerged LoRA adapters, produced by RUNNING THE REFERENCE's own unfused path
(`LoRALinear.forward`: frozen_W(x) + lora_B(lora_A(x)) * scaling, modules/lora.py:116-118; build container only:
`python tests/golden/make_golden_lm_lora.py <path to the reference's moshi package directory>`).

lm_lora.npz - tiny Moshi LM (moshi_amd.config.tiny_lm_config), bf16, seeded weights re-drawn from the stored seed, every nn.Linear
wrapped by `replace_all_linear_with_lora` (rank 32, scaling 2), B = 4 sessions, greedy, `support_out_of_sync=True`, three runs on
the same input codes: run 0 without an adapter (lora_B = 0), run 1 with adapter 0, run 2 with adapter 1.  The adapters are re-drawn
in the test from the stored seeds (tests/lora_cases.random_adapter).  For every run and step: the logits every token was sampled
from (recorded at `sample_token`) and the sampled tokens.

Adapter magnitudes: lora_A ~ N(0, A_STD^2 / in_features), lora_B ~ N(0, B_STD^2 / rank).  On a normalised input row (rms 1) the
update scaling * B (A x) of a linear then has a standard deviation of about scaling * A_STD * B_STD = 0.25, a quarter of the base
linear's own output (weights ~ N(0, 1 / in_features)): a strong fine-tune, still an UPDATE of the base model rather than a
replacement of it.  (With the update as large as the base output, A_STD = B_STD = 0.7, the engine sat at up to 5.3 % max / 2.0 %
mean of max|logit| from the reference in a few depth-transformer rows, against the gate's 5 % / 1.2 %.  The likely cause - not
measured - is that the reference's unfused path rounds to bf16 three times per linear where the engine rounds once.)  Every
adapted row's text logits must still be far from the base run's: asserted below against four times the gate of
tests/lm_cases.logits_close - the test on the engine fails without the feature.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
RANK, SCALING, A_STD, B_STD = 32, 2.0, 0.35, 0.35
ADAPTER_SEEDS = (101, 202)


def run(lm_gen, codes, B):
    import moshi.models.lm as lm_mod
    out = {"text_logits": [], "audio_logits": [], "text_tokens": [], "audio_tokens": []}
    rec = []
    orig = lm_mod.sample_token

    def sample_token(logits, *a, **k):
        tok = orig(logits, *a, **k)
        rec.append((logits.float().numpy().reshape(logits.shape[0], -1).copy(), tok.numpy().reshape(-1).copy()))
        return tok
    lm_mod.sample_token = sample_token
    try:
        with torch.no_grad(), lm_gen.streaming(B):
            for s in range(codes.shape[0]):
                rec.clear()
                lm_gen.step(torch.from_numpy(codes[s]))
                out["text_logits"].append(rec[0][0]); out["text_tokens"].append(rec[0][1])
                out["audio_logits"].append(np.stack([r[0] for r in rec[1:]], 1))
                out["audio_tokens"].append(np.stack([r[1] for r in rec[1:]], 1))
    finally:
        lm_mod.sample_token = orig
    return {k: np.stack(v) for k, v in out.items()}


def main():
    from moshi.models.lm import LMGen, LMModel
    from moshi.modules.lora import LoRALinear, replace_all_linear_with_lora
    from moshi_amd.config import tiny_lm_config
    from moshi_amd.weights import random_lm_state_dict
    from tests import lm_cases
    from tests.lora_cases import adapter_keys, random_adapter
    cfg = tiny_lm_config()
    seed = 83
    sd = random_lm_state_dict(cfg, seed=seed)
    B, S = 4, 5
    g = torch.Generator().manual_seed(17)
    codes = torch.randint(0, cfg.card, (S, B, cfg.n_q - cfg.dep_q, 1), generator=g).numpy()
    lm = LMModel(**cfg.reference_kwargs(), device="cpu", dtype=torch.bfloat16)
    lm.load_state_dict(sd, strict=True)
    replace_all_linear_with_lora(lm, RANK, SCALING)
    lm.eval()
    wrapped = {name: m for name, m in lm.named_modules() if isinstance(m, LoRALinear)}
    assert sorted(wrapped) == sorted(adapter_keys(sd)), "the reference wraps another set of linears than the engine adapts"

    def set_adapter(ad):
        with torch.no_grad():
            for name, m in wrapped.items():
                if ad is None:
                    m.lora_A.weight.zero_(); m.lora_B.weight.zero_()
                else:
                    m.lora_A.weight.copy_(ad[name + ".lora_A.weight"]); m.lora_B.weight.copy_(ad[name + ".lora_B.weight"])
    runs = []
    for ad_seed in (None,) + ADAPTER_SEEDS:
        set_adapter(None if ad_seed is None else random_adapter(sd, RANK, ad_seed, A_STD, B_STD))
        runs.append(run(LMGen(lm, use_sampling=False, support_out_of_sync=True), codes, B))
    out = {"seed": np.array([seed]), "rank": np.array([RANK]), "scaling": np.array([SCALING]), "a_std": np.array([A_STD]),
           "b_std": np.array([B_STD]), "adapter_seeds": np.array(ADAPTER_SEEDS), "codes": codes}
    out.update({k: np.stack([r[k] for r in runs]) for k in runs[0]})
    tl = out["text_logits"]
    margin = []
    for r in (1, 2):
        for s in range(S):
            for b in range(B):
                assert not lm_cases.logits_close(tl[r, s, b], tl[0, s, b], widen=4.0), (r, s, b)
                margin.append(float(np.abs(tl[r, s, b] - tl[0, s, b]).max() / (np.abs(tl[0, s, b]).max() + 1e-6)))
    print("adapted rows against the base run: max |d| / max|ref| between", min(margin), "and", max(margin),
          "(the gate of logits_close is", lm_cases.LOGIT_MAX_REL, ")")
    np.savez_compressed(HERE / "lm_lora.npz", **out)
    print("lm_lora.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOSHI_REFERENCE")
    assert ref, "usage: make_golden_lm_lora.py <directory that holds the reference's `moshi` package>"
    sys.path.insert(0, ref)
    sys.path.insert(0, str(HERE.parent.parent))
    main()
