"""ms per `LMGen.step` of one LM shape at a list of model-row counts, for the many-row handle (`LMModel(max_rows=)`, 65..128 rows)
and its yardstick, the <= 64-row handle.

    python scripts/bench_many_rows.py --shape 7b|tts --rows 64,96,128 [--steps 100] [--warmup 20] [--repeats 3] [--sites]

Shapes: the 7B benchmark model of bench_lm.py (seeded random weights, sampling on) and the TTS-family 1.6B shape of
scripts/bench_tts_lm.py (one 16-position cross condition).  Timing as bench_lm._time_lm_steps: a device-event pair around every
step; per repeat the median over `--steps` steps, reported as the median of the repeats with their min / max.  --sites adds the
per-site times of un-graphed steps (the profile tap) for the temporal in_proj and linear_in: a kernel inside the step, behind
its producer, not an independent launch.  MMI_* variables (MMI_ROWS_GROUPS=1: the control that launches the <= 64-row kernels
once per row group; MMI_ROWS_NTW) are read from the environment by the handle, as always.  Also runs from a checkout of an
earlier commit given as --root (its moshi_amd is imported; rows above 64 are then refused by that tree).  Prints ONE JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["7b", "tts"], default="7b")
    ap.add_argument("--rows", default="64,128")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sites", action="store_true")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    args = ap.parse_args()
    root = Path(args.root).resolve()
    sys.path.insert(0, str(root))
    sys.path.insert(0, str(root / "scripts"))
    from bench_lm import _time_lm_steps
    from moshi_amd import _capi
    from moshi_amd.config import LMConfig
    from moshi_amd.lm import ConditionFuser, LMGen, LMModel
    from moshi_amd.weights import random_lm_state_dict
    dev = torch.device("cuda:0")
    if args.shape == "7b":
        cfg = LMConfig()
        sd = random_lm_state_dict(cfg, seed=4242, device=dev)
    else:
        from bench_tts_lm import tts_16b_config
        cfg = tts_16b_config()
        sd = random_lm_state_dict(cfg, seed=0, device="cuda")
    res = {"metric": "lm_step_ms_by_rows", "shape": args.shape, "root": root.name, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "rows": {}}
    for B in [int(b) for b in args.rows.split(",")]:
        size = {"max_rows": B} if B > 64 else {"max_batch": B}
        kw, gkw = {}, dict(use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, seed=1234)
        if args.shape == "tts":
            kw["fuser"] = ConditionFuser({"cross": ["x"]})
            g = torch.Generator(device="cuda").manual_seed(1)
            x = (0.5 * torch.randn(B, 16, cfg.dim, generator=g, device="cuda")).to(torch.bfloat16)
            gkw = dict(use_sampling=True, condition_tensors={"x": (x, torch.ones(B, 16, dtype=torch.bool, device="cuda"))})
        lm = LMModel(sd, cfg, device=dev, **size, **kw)
        gen = LMGen(lm, **gkw)
        codes = torch.zeros(B, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=dev)
        entry = {}
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
                    site, n, tot, _ = ln.split("\t")
                    if site in ("L.in_proj", "L.ffn_in", "L.out_proj", "L.ffn_out"):
                        entry[site + "_us"] = round(1e3 * float(tot) / int(n), 2)
        res["rows"][str(B)] = entry
        del gen, lm
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
