"""What chunked prefill (mmi_lm_prefill) buys: the time to put T known frames into one fresh session of the 7B shape
(random weights) by `LMGen.prefill` on this tree, against the same frames through forced `step`s of a one-session handle on another
checkout (`--root`, the parent commit: what a user has today).  Device events around the whole fill, median of repeats with min / max.

    python scripts/bench_prefill.py --root <parent checkout> [--T 1024,3000] [--rounds 2]

runs the two sides alternately, `--rounds` times each, every run in a process of its own (a tree is importable once per process), and
prints one JSON line; the distance between two runs of the same side is the spread.

    python scripts/bench_prefill.py --child prefill|steps [--root DIR] ...       # one side, one JSON line
    python scripts/bench_prefill.py --child pass --depths 0,1024,2872            # ms of ONE 128-row pass at those ring depths
    python scripts/bench_prefill.py --kernel-trace <rocprofv3 *_kernel_trace.csv>   # microseconds per kernel name of such a run

The last form reads the kernel trace of a `--child pass` run made under `rocprofv3 --kernel-trace`: per kernel name, the median
duration of its launches per pass (the passes are told apart by the k_pf_prepare launches that open them)."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def child(args):
    root = Path(args.root).resolve() if args.root else HERE
    sys.path.insert(0, str(root))
    import torch
    from moshi_amd.config import LMConfig
    from moshi_amd.lm import LMGen, LMModel
    from moshi_amd.weights import random_lm_state_dict
    dev = torch.device("cuda:0")
    cfg = LMConfig()
    if args.layers:
        cfg.num_layers = args.layers
    sd = random_lm_state_dict(cfg, seed=4242, device=dev)
    size = dict(max_batch=1) if args.child == "steps" else dict(max_rows=128, prefill_rows=128)
    lm = LMModel(sd, cfg, device=dev, **size)
    del sd
    torch.cuda.empty_cache()
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    n_user, nq = cfg.n_q - cfg.dep_q, 1 + cfg.dep_q
    g = torch.Generator(device="cpu").manual_seed(1)
    out = {"side": args.child, "root": str(root), "layers": cfg.num_layers}

    def frames(T):
        codes = torch.randint(0, cfg.card, (1, n_user, T), generator=g).to(dev)
        toks = torch.cat([torch.randint(0, cfg.text_card, (1, 1, T), generator=g), torch.randint(0, cfg.card, (1, cfg.dep_q, T), generator=g)], 1).to(dev)
        return codes, toks

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b)
    with gen.streaming(1):
        if args.child == "pass":
            codes, toks = frames(128)
            res = {}
            for depth in [int(v) for v in args.depths.split(",")]:
                ms = []
                for _ in range(args.repeats + 1):
                    gen.seek([depth])
                    ms.append(timed(lambda: gen.prefill(codes, toks)))
                res[str(depth)] = _stats(ms[1:])                    # the first run of a depth warms up
            out["pass_ms_by_depth"] = res
        else:
            res = {}
            for T in [int(v) for v in args.T.split(",")]:
                codes, toks = frames(T)
                ms = []
                for _ in range(args.repeats):
                    gen.reset_streaming()
                    if args.child == "prefill":
                        ms.append(timed(lambda: gen.prefill(codes, toks)))
                    else:
                        def run():
                            for f in range(T):
                                gen._step(codes[:, :, f:f + 1], False, None, toks[:, :, f])
                        ms.append(timed(run))
                res[str(T)] = dict(_stats(ms), passes=(T + 127) // 128 if args.child == "prefill" else T)
            out["fill_ms_by_T"] = res
    print(json.dumps(out), flush=True)


def kernel_trace(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    passes, cur = [], None
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        if name.startswith("k_pf_prepare"):
            cur = {}
            passes.append(cur)
        if cur is not None:
            cur.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    out = []
    for i, p in enumerate(passes):
        out.append({"pass": i, "kernels": {k: {"launches": len(v), "median_us": statistics.median(v), "total_us": sum(v)} for k, v in sorted(p.items())}})
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default="", help="the other checkout (the parent commit) whose forced steps are the yardstick")
    ap.add_argument("--child", default="", choices=["", "prefill", "steps", "pass"])
    ap.add_argument("--T", default="1024,3000")
    ap.add_argument("--depths", default="0,1024,2872")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer temporal layers (invalidates the result)")
    ap.add_argument("--kernel-trace", default="")
    args = ap.parse_args()
    if args.kernel_trace:
        return kernel_trace(args.kernel_trace)
    if args.child:
        return child(args)
    assert args.root, "--root <parent checkout> is the yardstick"
    runs = []
    common = ["--T", args.T, "--repeats", str(args.repeats)] + (["--layers", str(args.layers)] if args.layers else [])
    plan = [(side, extra) for _ in range(args.rounds) for side, extra in (("steps", ["--root", args.root]), ("prefill", []))]
    for side, extra in plan:
        # a child that did not end well (a fault, an abort, a time limit) ends the session: nothing more is started on the card
        try:
            p = subprocess.run([sys.executable, __file__, "--child", side] + extra + common, capture_output=True, text=True, timeout=1500)
        except subprocess.TimeoutExpired:
            print(json.dumps({"runs": runs, "error": f"the {side} child ran into its time limit; stopped"}), flush=True)
            sys.exit(124)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            print(json.dumps({"runs": runs, "error": f"the {side} child ended with status {p.returncode}; stopped", "stderr": p.stderr[-400:]}), flush=True)
            sys.exit(p.returncode or 1)
        runs.append(json.loads(line[-1]))
    res = {"runs": runs}
    ok = [r for r in runs if "fill_ms_by_T" in r]
    for T in args.T.split(","):
        st = [r["fill_ms_by_T"][T]["median_ms"] for r in ok if r["side"] == "steps"]
        pf = [r["fill_ms_by_T"][T]["median_ms"] for r in ok if r["side"] == "prefill"]
        if st and pf:
            res[f"T={T}"] = {"steps_ms": st, "prefill_ms": pf, "ratio": statistics.mean(st) / statistics.mean(pf),
                             "spread_steps_ms": max(st) - min(st), "spread_prefill_ms": max(pf) - min(pf),
                             "ms_per_pass": statistics.mean(pf) / ((int(T) + 127) // 128)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
