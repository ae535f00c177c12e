"""What teacher-forced scoring on the prefill path (mmi_lm_score) buys: the time to get the model's logits over T known
frames of one fresh session of the 7B shape (random weights) by `LMGen.score` on this tree, against the same frames through forced
`step_with_taps` steps of a one-session handle on another checkout (`--root`, the parent commit: the only way it yields these logits).
Device events around the whole call, median of repeats with min / max.

    python scripts/bench_score.py --root <parent checkout> [--T 128,1024] [--rounds 2]

runs the sides alternately, `--rounds` times each, every run in a process of its own (a tree is importable once per process), and
prints one JSON line; the distance between two runs of the same side is the spread.

    python scripts/bench_score.py --child steps|score|score_logits|prefill [--root DIR] ...      # one side, one JSON line
    python scripts/bench_score.py --kernel-trace <rocprofv3 *_kernel_trace.csv>                  # microseconds per kernel name

`score` is commit = 1 without the fp32 logits, `score_logits` with them; `prefill` is `LMGen.prefill` of the same frames on this tree
(score minus prefill = the last layer's tail, the heads, the depth transformer and the output kernel).  The last form reads the kernel
trace of a `--child score` run made under `rocprofv3 --kernel-trace`: per kernel name, launches, median and total microseconds of
one pass (the passes are told apart by the k_pf_prepare launches that open them; the last pass of the trace is reported)."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
SIDES = ("steps", "score", "score_logits", "prefill")


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
    size = {"steps": dict(max_batch=1), "prefill": dict(max_rows=128, prefill_rows=128)}.get(args.child, dict(max_rows=128, prefill_rows=128, score=True))
    lm = LMModel(sd, cfg, device=dev, **size)
    del sd
    torch.cuda.empty_cache()
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    n_user = cfg.n_q - cfg.dep_q
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
        res = {}
        for T in [int(v) for v in args.T.split(",")]:
            codes, toks = frames(T)
            ms = []
            for _ in range(args.repeats + 1):
                gen.reset_streaming()
                if args.child == "prefill":
                    ms.append(timed(lambda: gen.prefill(codes, toks)))
                elif args.child == "steps":
                    def run():
                        for f in range(T):
                            gen.step_with_taps(codes[:, :, f:f + 1], forced_tokens=toks[:, :, f])
                    ms.append(timed(run))
                else:
                    ms.append(timed(lambda: gen.score(codes, toks, commit=True, return_logits=args.child == "score_logits")))
            res[str(T)] = _stats(ms[1:])                                # the first run of a length warms up
        out["ms_by_T"] = res
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
    p = passes[-1]
    kern = {k: {"launches": len(v), "median_us": statistics.median(v), "total_us": sum(v)} for k, v in sorted(p.items())}
    print(json.dumps({"passes_in_trace": len(passes), "pass": len(passes) - 1, "total_us": sum(k["total_us"] for k in kern.values()), "kernels": kern}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default="", help="the other checkout (the parent commit) whose forced steps are the yardstick")
    ap.add_argument("--child", default="", choices=("",) + SIDES)
    ap.add_argument("--T", default="128,1024")
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
    plan = [(side, ["--root", args.root] if side == "steps" else []) for _ in range(args.rounds) for side in SIDES]
    for side, extra in plan:
        # a child that did not end well (a fault, an abort, a time limit) ends the session: nothing more is started on the card
        try:
            p = subprocess.run([sys.executable, __file__, "--child", side] + extra + common, capture_output=True, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            print(json.dumps({"runs": runs, "error": f"the {side} child ran into its time limit; stopped"}), flush=True)
            sys.exit(124)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            print(json.dumps({"runs": runs, "error": f"the {side} child ended with status {p.returncode}; stopped", "stderr": p.stderr[-400:]}), flush=True)
            sys.exit(p.returncode or 1)
        runs.append(json.loads(line[-1]))
        print(f"# {side}: {line[-1]}", file=sys.stderr, flush=True)
    res = {"runs": runs}
    for T in args.T.split(","):
        by = {side: [r["ms_by_T"][T]["median_ms"] for r in runs if r["side"] == side] for side in SIDES}
        if all(by.values()):
            mean = {k: statistics.mean(v) for k, v in by.items()}
            res[f"T={T}"] = {**{f"{k}_ms": v for k, v in by.items()}, **{f"spread_{k}_ms": max(v) - min(v) for k, v in by.items()},
                             "steps_over_score": mean["steps"] / mean["score"], "steps_over_score_logits": mean["steps"] / mean["score_logits"],
                             "score_minus_prefill_ms": mean["score"] - mean["prefill"]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
