"""What per-session LoRA adapters cost inside `LMGen.step`: ms per step at the 7B shape, random weights, one box,
for four handles at each batch -

  plain        a plain handle
  unfused      a plain handle under the knobs that select an adapter handle's launch list minus its shrink launches
               (MMI_GEMM_LDS=0 MMI_GEMM_ONCE=0 MMI_NO_NORM_FUSION MMI_NO_DEP_ATTN_FUSION MMI_NO_DEP_IN_GROUP)
  adapters_off an adapter handle (4 slots of rank 128) with every row at -1
  adapters_on  the same with four rank-128 adapters spread over the rows

`adapters_off - unfused` is the price of the shrink launches and the tail, `unfused - plain` the price of leaving the fused forms.
One JSON line per (case, batch): graph-replayed ms per step (median of `--repeats` timings of `--steps` steps) and, from
`mmi_lm_profile_sites` on un-graphed steps, the time of the shrink sites and of the linears behind them.

    python scripts/bench_lora.py [--sessions 1,32] [--steps 60] [--warmup 20] [--layers 32]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
from contextlib import contextmanager
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from moshi_amd import LMGen, LMModel, _capi  # noqa: E402
from moshi_amd.config import LMConfig  # noqa: E402
from moshi_amd.weights import is_lm_linear_weight, random_lm_state_dict  # noqa: E402

UNFUSED = {"MMI_GEMM_LDS": "0", "MMI_GEMM_ONCE": "0", "MMI_NO_NORM_FUSION": "1", "MMI_NO_DEP_ATTN_FUSION": "1", "MMI_NO_DEP_IN_GROUP": "1"}


@contextmanager
def env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def adapter(sd, rank, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for key in [k for k in sd if is_lm_linear_weight(k)]:
        N, K = sd[key].shape
        stem = key[: -len(".weight")]
        out[stem + ".lora_A.weight"] = (torch.randn(rank, K, generator=g, device=dev) * (0.35 / K ** 0.5)).to(torch.bfloat16)
        out[stem + ".lora_B.weight"] = (torch.randn(N, rank, generator=g, device=dev) * (0.35 / rank ** 0.5)).to(torch.bfloat16)
    return out


def time_steps(gen, codes, steps, warmup, repeats):
    for _ in range(warmup):
        gen.step(codes)
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            gen.step(codes)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return sorted(ms)


def site_times(gen, codes, n=10):
    lib, h = gen._lib, gen.lm_model._handle
    torch.cuda.synchronize()
    lib.check(lib.mmi_lm_profile_begin(h))
    for _ in range(n):
        gen.step(codes)
    torch.cuda.synchronize()
    txt = _capi.read_text(lambda buf, cap: lib.mmi_lm_profile_sites(h, buf, cap))
    mean_ms, cnt, nbytes, name = C.c_double(), C.c_int64(), C.c_int64(), C.c_char_p()
    lib.check(lib.mmi_lm_profile_end(h, C.byref(mean_ms), C.byref(cnt), C.byref(nbytes), C.byref(name)))
    out = {}
    for line in txt.splitlines():
        f = line.split("\t")
        if len(f) >= 3 and int(f[1]) > 0:
            out[f[0]] = {"ops_per_step": int(f[1]) / n, "us_per_op": round(1e3 * float(f[2]) / int(f[1]), 2), "us_per_step": round(1e3 * float(f[2]) / n, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,32")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--cases", default="plain,unfused,adapters_off,adapters_on")
    args = ap.parse_args()
    dev = torch.device("cuda")
    from dataclasses import replace
    cfg = replace(LMConfig(), num_layers=args.layers)
    sd = random_lm_state_dict(cfg, seed=0, device=dev)
    ads = None
    for B in [int(v) for v in args.sessions.split(",")]:
        codes = torch.randint(0, cfg.card, (B, cfg.n_q - cfg.dep_q, 1), device=dev)
        for case in args.cases.split(","):
            with env(UNFUSED if case == "unfused" else {}):
                lm = LMModel(sd, cfg, device=dev, max_batch=B, adapters=(4, 128) if case.startswith("adapters") else None)
            if case == "adapters_on":
                if ads is None:
                    ads = [adapter(sd, 128, 100 + j, dev) for j in range(4)]
                for j, ad in enumerate(ads):
                    lm.load_adapter(j, ad, scaling=2.0)
            gen = LMGen(lm, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, seed=1234)
            with gen.streaming(B):
                if case == "adapters_on":
                    for b in range(B):
                        gen.set_session_adapter(b, b % 4)
                ms = time_steps(gen, codes, args.steps, args.warmup, args.repeats)
                sites = site_times(gen, codes)
                launches = len(gen.launch_list())
            shrink = {k: v for k, v in sites.items() if k.endswith(".lora")}
            rec = {"case": case, "sessions": B, "layers": args.layers, "ms_per_step": round(ms[len(ms) // 2], 4), "ms_per_step_all": [round(v, 4) for v in ms],
                   "launches_per_step": launches, "shrink_us_per_step": round(sum(v["us_per_step"] for v in shrink.values()), 1),
                   "sites_us_per_op": {k: v["us_per_op"] for k, v in sites.items() if k.endswith(".lora") or k + ".lora" in sites or case in ("plain", "unfused") and
                                       k in ("L.in_proj", "L.out_proj", "L.ffn_in", "L.ffn_out", "text_linear", "dep.in", "dep.in_all", "dep.in_proj", "dep.out_proj",
                                             "dep.ffn_in", "dep.ffn_out", "dep.lin")}}
            print(json.dumps(rec), flush=True)
            del gen, lm
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
