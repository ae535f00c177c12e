"""ms per `LMGen.step` of the 7B shape with the nucleus samplers, at 1 and 32 sessions, in three configurations:
not enabled (k_sample), enabled with every value 0 (k_sample_nucleus on its top-k paths), and top_p = top_p_text = 0.9 on the handle
with the sessions' own values spread over 0.5 .. 0.99: `python scripts/bench_top_p.py [--steps 60 --warmup 12 --batches 1,32]`.
`--configs` picks among not_enabled, enabled_zero, top_p, spread (a kernel trace of one configuration alone).  Prints one JSON line
per batch size.  The model, the ring depth and the timing loop are bench.py's `--workload lm`."""
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
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--configs", default="not_enabled,enabled_zero,top_p,spread,not_enabled_again")
    ap.add_argument("--lm-layers", type=int, default=0)
    ap.add_argument("--quant", default="none")
    ap.add_argument("--kv", default="bf16")
    args = ap.parse_args()
    from bench_lm import make_lm
    from moshi_amd.lm import LMGen
    dev = torch.device("cuda", 0)
    batches = [int(b) for b in args.batches.split(",")]
    lm = make_lm(dev, max(batches), args, streaming=False)
    for B in batches:
        codes = torch.randint(0, 2048, (B, 8, 1), device=dev, generator=torch.Generator(device=dev).manual_seed(1000))

        def timed(spread=False, **kw):
            gen = LMGen(lm, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, seed=1234, **kw)
            with gen.streaming(B):
                gen.seek([250 + 8 * b for b in range(B)])
                if spread:
                    for b in range(B):
                        p = 0.5 + 0.49 * b / max(1, B - 1)
                        gen.set_session_top_p(b, p, p)
                for _ in range(args.warmup):
                    gen.step(codes)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    gen.step(codes)
                torch.cuda.synchronize(dev)
                return 1e3 * (time.perf_counter() - t0) / args.steps
        runs = {"not_enabled": lambda: timed(), "enabled_zero": lambda: timed(session_top_p=True),
                "top_p": lambda: timed(top_p=0.9, top_p_text=0.9), "spread": lambda: timed(spread=True, top_p=0.9, top_p_text=0.9),
                "not_enabled_again": lambda: timed()}
        out = {"batch": B, "steps": args.steps}
        for name in args.configs.split(","):
            out["ms_per_step_" + name] = runs[name]()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
