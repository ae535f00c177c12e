"""Step time of a TTS-family LM (kyutai's TTS checkpoints: n_q = dep_q = 32, depformer weight schedule, low-rank depformer
embeddings, demuxed text stream, cross-attention) on the engine.

    python scripts/bench_tts_lm.py [--batches 1,8,32] [--steps 200] [--warmup 20]

The model has the 1.6B shape modelled on the published TTS configuration (dim 2048 x 16 layers, depformer 1024 x 4 layers, 32
micro-steps over 9 weight sets, rank 128) with seeded random weights: nothing is downloaded and the exact published values
are not verified here.  ms per `LMGen.step` from device events over `--steps` steps after `--warmup`, sampling on, one
16-position `cross` condition.  Prints ONE JSON line; frames/s = B * 1000 / ms against the 12.5 Hz real-time rate.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def tts_16b_config():
    from moshi_amd.config import LMConfig
    return LMConfig(dim=2048, num_heads=16, num_layers=16, hidden_scale=4.125, context=500, n_q=32, dep_q=32, card=2048, text_card=8000,
                    depformer_dim=1024, depformer_dim_feedforward=int(4.125 * 1024), depformer_num_heads=16, depformer_num_layers=4,
                    delays=[0] + [2] * 32, cross_attention=True, depformer_weights_per_step_schedule=list(range(8)) + [8] * 24,
                    depformer_low_rank_embeddings=128, demux_second_text_stream=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from moshi_amd.lm import ConditionFuser, LMGen, LMModel
    from moshi_amd.weights import random_lm_state_dict
    cfg = tts_16b_config()
    sd = random_lm_state_dict(cfg, seed=0, device="cuda")
    n_params = sum(v.numel() for v in sd.values())
    res = {"metric": "tts_lm_step_ms", "model": "tts-1.6b-shape (random init)", "params": n_params, "steps": args.steps,
           "warmup": args.warmup, "frame_rate_hz": 12.5, "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        lm = LMModel(sd, cfg, device="cuda", max_batch=B, fuser=ConditionFuser({"cross": ["x"]}))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = (0.5 * torch.randn(B, 16, cfg.dim, generator=g, device="cuda")).to(torch.bfloat16)
        gen = LMGen(lm, use_sampling=True, condition_tensors={"x": (x, torch.ones(B, 16, dtype=torch.bool, device="cuda"))})
        codes = torch.zeros(B, 0, 1, dtype=torch.int64, device="cuda")
        with gen.streaming(B):
            for _ in range(args.warmup):
                gen.step(codes)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                gen.step(codes)
            t1.record()
            torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.steps
        res["batches"][str(B)] = {"ms_per_step": round(ms, 4), "frames_per_s": round(B * 1000.0 / ms, 1),
                                  "x_real_time": round(1000.0 / ms / 12.5, 1)}
        del gen, lm
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
