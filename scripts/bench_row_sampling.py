"""ms per LM step at 32 sessions with every row on its own sampling settings (own seed, repetition_context = 32, pad_mult != 0)
against the same stream with no row active: `python scripts/bench_row_sampling.py [--steps 60 --warmup 12 --batch 32]`.
Prints one JSON line.  The model, the ring depth and the timing loop are bench.py's `--workload lm`."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lm-layers", type=int, default=0)
    ap.add_argument("--quant", default="none")
    ap.add_argument("--kv", default="bf16")
    args = ap.parse_args()
    from bench_lm import make_lm
    from moshi_amd import SessionSampling
    dev = torch.device("cuda", 0)
    B = args.batch
    gen = make_lm(dev, B, args)
    codes = torch.randint(0, 2048, (B, 8, 1), device=dev, generator=torch.Generator(device=dev).manual_seed(1000))
    gen.seek([250 + 8 * b for b in range(B)])

    def timed():
        for _ in range(args.warmup):
            gen.step(codes)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            gen.step(codes)
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0) / args.steps
    out = {"batch": B, "steps": args.steps}
    out["ms_per_step_inactive"] = timed()
    gen.set_session_sampling([SessionSampling(seed=100 + b, repetition_penalty=1.3, repetition_context=32, pad_mult=0.5) for b in range(B)])
    out["ms_per_step_all_active"] = timed()
    gen.clear_session_sampling()
    out["ms_per_step_inactive_again"] = timed()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
