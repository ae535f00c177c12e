"""ms per `mmi_lm_streaming_start` + synchronise of the 7B shape at bench.py's configuration (32 sessions, bf16, top_k 250 / 25), by
a host clock: `python scripts/bench_streaming_start.py [--batch 32 --repeats 3]`.  The call is the stream's device allocations, its
fills and the step program's build; the stop between two starts is not timed.  Prints one JSON line.  For a same-box A/B of two
builds name the other library with MMI_LIB_PATH and alternate the processes (profiles/state_table/README.md)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lm-layers", type=int, default=0)
    ap.add_argument("--quant", default="none")
    ap.add_argument("--kv", default="bf16")
    args = ap.parse_args()
    from bench_lm import make_lm
    from moshi_amd.lm import LMGen
    dev = torch.device("cuda", 0)
    lm = make_lm(dev, args.batch, args, streaming=False)
    gen = LMGen(lm, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, seed=1234)
    ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        gen.streaming_forever(args.batch)
        torch.cuda.synchronize(dev)
        ms.append(1e3 * (time.perf_counter() - t0))
        gen._stop_streaming()
    print(json.dumps({"metric": "streaming_start", "batch": args.batch, "ms": [round(v, 3) for v in ms],
                      "median_ms": round(statistics.median(ms), 3)}), flush=True)


if __name__ == "__main__":
    main()
