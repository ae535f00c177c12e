"""Time of one `LMGen.set_session_condition` (mmi_lm_set_row_condition) on the TTS-shaped LM of scripts/bench_tts_lm.py: a
128-position cross-attention source for one session of a live stream, device events around the call alone.  It is paid once per
session, not per step.  Prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--positions", type=int, default=128)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    from bench_tts_lm import tts_16b_config
    from moshi_amd.lm import ConditionFuser, LMGen, LMModel, SessionCondition
    from moshi_amd.weights import random_lm_state_dict
    cfg = tts_16b_config()
    B, L = args.batch, args.positions
    lm = LMModel(random_lm_state_dict(cfg, seed=0, device="cuda"), cfg, device="cuda", max_batch=B, fuser=ConditionFuser({"cross": ["x"]}),
                 cross_capacity=L)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (0.5 * torch.randn(B, 16, cfg.dim, generator=g, device="cuda")).to(torch.bfloat16)
    own = (0.5 * torch.randn(1, L, cfg.dim, generator=g, device="cuda")).to(torch.bfloat16)
    cond = SessionCondition(condition_tensors={"x": (own, torch.ones(1, L, dtype=torch.bool, device="cuda"))})
    gen = LMGen(lm, use_sampling=True, condition_tensors={"x": (x, torch.ones(B, 16, dtype=torch.bool, device="cuda"))})
    codes = torch.zeros(B, 0, 1, dtype=torch.int64, device="cuda")
    times = []
    with gen.streaming(B):
        for i in range(args.calls + 3):
            gen.step(codes)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            gen.set_session_condition(i % B, cond)
            t1.record()
            torch.cuda.synchronize()
            if i >= 3:
                times.append(t0.elapsed_time(t1))
    times.sort()
    print(json.dumps({"metric": "set_row_condition_ms", "batch": B, "positions": L, "calls": len(times), "median_ms": round(times[len(times) // 2], 4),
                      "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4)}), flush=True)


if __name__ == "__main__":
    main()
