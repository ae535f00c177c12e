"""Shared checks of the TTS-family LM options (depformer weight schedule, low-rank depformer embeddings, demuxed text stream,
dep_q above 16, n_q == dep_q) against tests/golden/lm_tts.npz - run on the kernel simulator and on the GPU."""
from __future__ import annotations

import hashlib
from dataclasses import replace
from pathlib import Path

import numpy as np
import torch

from tests.lm_cases import GUIDED_WIDEN, logits_close
from moshi_amd.config import tiny_lm_config, tiny_tts_config
from moshi_amd.lm import ConditionFuser, LMGen, LMModel
from moshi_amd.weights import random_lm_state_dict

GOLDEN = Path(__file__).resolve().parent / "golden"


def h_config():
    return replace(tiny_lm_config(), depformer_weights_per_step_schedule=[0] + [1] * 7, depformer_low_rank_embeddings=16)


def state_dict_digest(sd) -> str:
    """sha256 over the names, shapes, dtypes and bytes of a state dict, in its order."""
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(f"{k}|{tuple(v.shape)}|{v.dtype}|".encode())
        h.update(v.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def check_tts_golden(device, lib, name):
    """Replays scenario `name` of lm_tts.npz on the engine, teacher-forced with the reference's sampled tokens (the hook and the
    replaced audio tokens applied on top, as in the reference's run): ring outputs identical, logits within tolerance."""
    g = np.load(GOLDEN / "lm_tts.npz")
    S, B = g["masks"].shape
    if name == "g":
        cfg = tiny_tts_config()
        t = lambda k: torch.from_numpy(g[k]).to(torch.bfloat16)
        conds = {"s": (t("g_sum"), torch.ones(2 * B, 1, dtype=torch.bool)), "x": (t("g_cross"), torch.ones(2 * B, g["g_cross"].shape[1], dtype=torch.bool))}
        fuser = ConditionFuser({"sum": ["s"], "cross": ["x"]})
        rows, coef, no_text = 2 * B, 2.0, True
    else:
        cfg, conds, fuser, rows, coef, no_text = h_config(), None, None, B, 1.0, False
    sd = random_lm_state_dict(cfg, seed=int(g[f"{name}_seed"][0]))
    lm = LMModel(sd, cfg, device=device, max_batch=rows, lib=lib, fuser=fuser)
    step = {"s": 0}
    hook = None
    if name == "g":
        def hook(tok):
            h = torch.from_numpy(g["g_hook"][step["s"]]).to(tok.device)
            tok.copy_(torch.where(h >= 0, h, tok))
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=coef, cfg_is_no_text=no_text, condition_tensors=conds,
                on_text_hook=hook)
    wd = GUIDED_WIDEN if coef != 1.0 else 1.0
    gen.streaming_forever(B)
    try:
        for s in range(S):
            step["s"] = s
            if s == int(g["reset_step"][0]):
                gen.reset_streaming(torch.from_numpy(g["reset_mask"]).to(device))
            gen.set_exec_mask(torch.from_numpy(g["masks"][s]).to(device))
            forced = np.concatenate([g[f"{name}_text_tok"][s][:, None], g[f"{name}_audio_tok"][s]], 1)
            out, tl, al = gen.step_with_taps(torch.from_numpy(g[f"{name}_codes"][s]).to(device),
                                             forced_tokens=torch.from_numpy(forced).to(device))
            out, tl, al = out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy()
            for b in range(B):
                if not g["masks"][s, b]:
                    continue
                assert np.array_equal(out[b], g[f"{name}_tokens"][s, b]), f"{name} step {s} row {b}: ring output differs"
                assert logits_close(tl[b], g[f"{name}_text_logits"][s, b]), f"{name} step {s} row {b}: text logits"
                if g[f"{name}_audio_valid"][s]:
                    for k in range(cfg.dep_q):
                        assert logits_close(al[b, k], g[f"{name}_audio_logits"][s, b, k], wd), f"{name} step {s} row {b} cb {k}: audio logits"
    finally:
        gen._stop_streaming()
    return S
