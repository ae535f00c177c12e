"""ms per `LMGen.step` of the 7B benchmark shape with bf16, int8 and OCP MXFP4 linears at a list of session counts.

    python scripts/bench_mxfp4.py [--formats bf16,int8,mxfp4] [--sessions 1,32,64] [--steps 100] [--warmup 20] [--repeats 3]
                                  [--rounds 2] [--sites]

Seeded random weights (bench_lm.py's model), sampling on.  Timing as bench_lm._time_lm_steps: a device-event pair around every
step; per repeat the median over `--steps` steps, reported as the median of the repeats with their min / max.  Every
(format, sessions) configuration runs `--rounds` times, the formats alternating inside a round, in one process on one card: the
distance between two rounds of the same configuration is the spread a difference between formats has to exceed.  --sites adds
the per-site times of un-graphed steps (the profile tap) for the temporal linears, with the weight bytes the launch streams and
the GB/s that makes: a kernel inside the step, behind its producer, not an independent launch.  Also runs from a checkout of
an earlier commit given as --root (its moshi_amd is imported; mxfp4 is then refused by that tree).  Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="bf16,int8,mxfp4")
    ap.add_argument("--sessions", default="1,32,64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sites", action="store_true")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    args = ap.parse_args()
    root = Path(args.root).resolve()
    sys.path.insert(0, str(root))
    sys.path.insert(0, str(root / "scripts"))
    from bench_lm import _time_lm_steps
    from moshi_amd import _capi, weights
    from moshi_amd.config import LMConfig
    from moshi_amd.lm import LMGen, LMModel
    dev = torch.device("cuda:0")
    cfg = LMConfig()
    bf16 = weights.random_lm_state_dict(cfg, seed=4242, device=dev)
    quantisers = {"bf16": lambda sd: sd, "int8": weights.quantize_lm_state_dict,
                  "mxfp4": getattr(weights, "quantize_lm_state_dict_mxfp4", None)}
    res = {"metric": "lm_step_ms_by_weight_format", "root": root.name, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "rounds": []}
    sds = {}
    for fmt in args.formats.split(","):
        if quantisers.get(fmt) is None:
            raise SystemExit(f"this tree has no {fmt} linears")
        sds[fmt] = quantisers[fmt](bf16)
    for rnd in range(args.rounds):
        this = {}
        for fmt, sd in sds.items():
            for B in [int(b) for b in args.sessions.split(",")]:
                lm = LMModel(sd, cfg, device=dev, max_batch=B)
                gen = LMGen(lm, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, seed=1234)
                codes = torch.zeros(B, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=dev)
                with gen.streaming(B):
                    meds = []
                    for r in range(args.repeats):
                        _, ms = _time_lm_steps(gen, codes, args.warmup if r == 0 else 5, args.steps, dev)
                        meds.append(statistics.median(ms))
                    entry = {"ms_per_step": round(statistics.median(meds), 4), "min": round(min(meds), 4), "max": round(max(meds), 4),
                             "kernels": sorted({k for _, k in gen.launch_list() if k.startswith("k_gemm")})}
                    if args.sites:
                        lib, h = gen._lib, lm._handle
                        torch.cuda.synchronize(dev)
                        lib.check(lib.mmi_lm_profile_begin(h))
                        for _ in range(20):
                            gen.step(codes)
                        torch.cuda.synchronize(dev)
                        txt = _capi.read_text(lambda buf, cap: lib.mmi_lm_profile_sites(h, buf, cap))
                        lib.check(lib.mmi_lm_profile_end(h, None, None, None, None))
                        for ln in txt.splitlines():
                            site, n, tot, nbytes = ln.split("\t")
                            if site in ("L.in_proj", "L.ffn_in", "L.out_proj", "L.ffn_out"):
                                us = 1e3 * float(tot) / int(n)
                                entry[site] = {"us": round(us, 2), "weight_bytes": int(nbytes), "GBps": round(int(nbytes) / us / 1e3, 1)}
                this[f"{fmt}/{B}"] = entry
                del gen, lm
                torch.cuda.empty_cache()
        res["rounds"].append(this)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
