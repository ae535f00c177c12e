"""ms per `LMGen.step` of the 7B benchmark model at given KV ring depths, for the three ring formats (`kv_cache_dtype` "bf16",
"fp8", "fp4"), and what the decode attention achieves in bytes per second.

    python scripts/bench_kv_ring.py [--sessions 32] [--depths 375,1500,3000] [--rings bf16,fp8,fp4,bf16,fp8,fp4]
                                    [--quantize] [--steps 200] [--warmup 20] [--repeats 5] [--sites]

Seeded random weights, sampling on (bench_lm.py's model); bf16 linears, or int8 with --quantize (the `c5` shape at 64 sessions).
Every session is moved with `mmi_lm_seek` (the skipped positions read the zeroed ring: same bytes streamed) to a position from
which the repeat's median step, and the middle of the tapped steps, sits at the named depth; at the full depth the ring is full
throughout.
Timing as bench_lm._time_lm_steps: a device-event pair around every step; per repeat the median over --steps steps, reported as
the median / min / max over --repeats repeats.  The rings are run in the order given, each handle built, timed at every depth and
released - name a ring twice to get the distance between two runs of the same ring, which is the spread a difference between
rings has to exceed.  --sites adds the per-site time of the decode attention launch (`L.attn`, un-graphed steps, the profile
tap) and from it the ring bytes it streams per second: 2 (keys, values) x sessions x heads x depth x head dim x bytes per element
(bf16 2, fp8 1, fp4 0.5625) per layer.  Also prints `mmi_lm_state_bytes` per session.  ONE JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

BYTES_PER_ELEMENT = {"bf16": 2.0, "fp8": 1.0, "fp4": 0.5625}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=32)
    ap.add_argument("--depths", default="375,1500,3000")
    ap.add_argument("--rings", default="bf16,fp8,fp4,bf16,fp8,fp4")
    ap.add_argument("--quantize", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sites", action="store_true")
    args = ap.parse_args()
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root))
    from bench_lm import _time_lm_steps
    from moshi_amd import _capi
    from moshi_amd.config import LMConfig
    from moshi_amd.lm import LMGen, LMModel
    from moshi_amd.weights import random_lm_state_dict
    dev = torch.device("cuda:0")
    B = args.sessions
    base = LMConfig()
    sd = random_lm_state_dict(base, seed=4242, device=dev)
    if args.quantize:
        from moshi_amd.weights import quantize_lm_state_dict
        sd = quantize_lm_state_dict(sd)
    depths = [int(d) for d in args.depths.split(",")]
    res = {"metric": "lm_step_ms_by_kv_ring", "sessions": B, "quantize": bool(args.quantize), "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "runs": []}
    for ring in args.rings.split(","):
        from dataclasses import replace
        cfg = replace(base, kv_cache_dtype=ring)
        lm = LMModel(sd, cfg, device=dev, max_batch=B)
        gen = LMGen(lm, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, seed=1234)
        codes = torch.zeros(B, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=dev)
        run = {"ring": ring, "depths": {}}
        with gen.streaming(B):
            run["state_bytes_per_session"] = int(gen._lib.mmi_lm_state_bytes(lm._handle)) // B
            for depth in depths:
                meds = []
                for r in range(args.repeats):
                    warm = args.warmup if r == 0 else 5
                    gen.seek([max(0, depth - warm - args.steps // 2)] * B)       # the median step of the repeat sits at `depth`
                    _, ms = _time_lm_steps(gen, codes, warm, args.steps, dev)
                    meds.append(statistics.median(ms))
                entry = {"ms_per_step": round(statistics.median(meds), 4), "min": round(min(meds), 4), "max": round(max(meds), 4)}
                if args.sites:
                    lib, h = gen._lib, lm._handle
                    gen.seek([max(0, depth - 10)] * B)                         # the 20 tapped steps straddle `depth`
                    torch.cuda.synchronize(dev)
                    lib.check(lib.mmi_lm_profile_begin(h))
                    for _ in range(20):
                        gen.step(codes)
                    torch.cuda.synchronize(dev)
                    txt = _capi.read_text(lambda buf, cap: lib.mmi_lm_profile_sites(h, buf, cap))
                    lib.check(lib.mmi_lm_profile_end(h, None, None, None, None))
                    for ln in txt.splitlines():
                        site, n, tot, _ = ln.split("\t")
                        if site in ("L.attn", "L.in_proj"):
                            entry[site + "_us"] = round(1e3 * float(tot) / int(n), 2)
                    if "L.attn_us" in entry:
                        rows = min(depth, cfg.context)
                        nbytes = 2 * B * cfg.dim * rows * BYTES_PER_ELEMENT[ring]
                        entry["attn_TB_per_s"] = round(nbytes / (entry["L.attn_us"] * 1e-6) / 1e12, 3)
                run["depths"][str(depth)] = entry
        res["runs"].append(run)
        del gen, lm
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
