"""What the log-probabilities of the live step (mmi_lm_enable_logprobs) cost: milliseconds per `LMGen.step` of the 7B
shape (random weights) at 1 and 32 sessions with the option off, with top_n = 0 and with top_n = 8 - one handle, one process, the
variants interleaved round by round, so that the yardstick is the same handle with the option off in the same run.  Device events
around `--steps` graphed steps after `--warmup`; per variant the median over the rounds with min / max.

    python scripts/bench_logprobs.py [--sessions 1,32] [--steps 200] [--warmup 30] [--rounds 5]
    python scripts/bench_logprobs.py --only top8 --sessions 32 --rounds 1       # one variant: the run to put under rocprofv3 --kernel-trace --stats

prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
VARIANTS = {"off": None, "top0": 0, "top8": 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", choices=("",) + tuple(VARIANTS))
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer temporal layers (invalidates the result)")
    args = ap.parse_args()
    sys.path.insert(0, str(HERE))
    import torch
    from moshi_amd.config import LMConfig
    from moshi_amd.lm import LMGen, LMModel
    from moshi_amd.weights import random_lm_state_dict
    dev = torch.device("cuda:0")
    cfg = LMConfig()
    if args.layers:
        cfg.num_layers = args.layers
    sessions = [int(v) for v in args.sessions.split(",")]
    sd = random_lm_state_dict(cfg, seed=4242, device=dev)
    lm = LMModel(sd, cfg, device=dev, max_batch=max(sessions))
    del sd
    torch.cuda.empty_cache()
    g = torch.Generator(device="cpu").manual_seed(1)
    variants = [args.only] if args.only else list(VARIANTS)
    ms = {(n, v): [] for n in sessions for v in variants}
    for n in sessions:
        codes = torch.randint(0, cfg.card, (n, cfg.n_q - cfg.dep_q, 1), generator=g).to(dev)
        for _ in range(args.rounds):
            for v in variants:
                gen = LMGen(lm, use_sampling=True, seed=7, support_out_of_sync=True, logprobs=VARIANTS[v])
                with gen.streaming(n):
                    for _ in range(args.warmup):
                        gen.step(codes)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(dev)
                    a.record()
                    for _ in range(args.steps):
                        gen.step(codes)
                    b.record()
                    torch.cuda.synchronize(dev)
                    ms[(n, v)].append(a.elapsed_time(b) / args.steps)
                    if VARIANTS[v] is not None:
                        assert torch.isfinite(gen.last_logprobs().logp).all()
    out = {"layers": cfg.num_layers, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": {}}
    for n in sessions:
        row = {v: {"median": statistics.median(ms[(n, v)]), "min": min(ms[(n, v)]), "max": max(ms[(n, v)])} for v in variants}
        if "off" in row:
            for v in variants:
                row[v]["over_off_us"] = 1000.0 * (row[v]["median"] - row["off"]["median"])
        out["ms_per_step"][str(n)] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
