"""What forking a session (mmi_lm_fork_session) costs at the 7B shape (random weights), and what it replaces: for the
bf16, e4m3 and 4-bit rings at ring depths 250, 1500 and 3000

  - microseconds per `LMGen.fork_session` to 1 and to 4 destinations (device events around the call, median of `--repeats` after
    warm-up calls), the bytes it read and wrote, and the resulting TB/s next to the read-only speed of light of DESIGN.md 10e
    (a copy moves its bytes twice);
  - in the same run, a plain device-to-device copy of as many bytes as the one-destination fork reads (what hipMemcpyAsync reaches);
  - in the same run, the alternative a user had before: `LMGen.prefill` of the same number of frames into one fresh session.

    python scripts/bench_fork.py [--rings bf16,fp8,fp4] [--depths 250,1500,3000] [--repeats 20]

One JSON line per (ring, depth), then one summary line.  One GPU, one process; every figure of a line comes from the same run."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
SOL_READ_TBS = 5.95          # the read-only speed of light measured on this part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", default="bf16,fp8,fp4")
    ap.add_argument("--depths", default="250,1500,3000")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=5, help="sessions of the stream: the source and four destinations")
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer temporal layers (invalidates the result)")
    ap.add_argument("--no-prefill", action="store_true")
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
    B = args.sessions
    n_user = cfg.n_q - cfg.dep_q
    H, Dh = cfg.num_heads, cfg.dim // cfg.num_heads
    g = torch.Generator(device="cpu").manual_seed(1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1000.0        # microseconds

    def stats(us):
        return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "n": len(us)}
    lines = []
    sd = random_lm_state_dict(cfg, seed=4242, device=dev)
    for ring in args.rings.split(","):
        lm = LMModel(sd, cfg, device=dev, max_rows=128, prefill_rows=128, kv_cache=ring)
        gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
        pos_bytes = {"bf16": 2 * Dh, "fp8": Dh, "fp4": Dh // 2 + Dh // 16}[ring]
        with gen.streaming(B):
            for depth in [int(v) for v in args.depths.split(",")]:
                valid = min(depth, cfg.context)
                read = 2 * cfg.num_layers * H * valid * pos_bytes          # keys and values, every layer and head, one model row
                gen.seek([depth] * B)                                      # the offsets alone: the copy moves the bytes whatever they hold
                line = {"ring": ring, "depth": depth, "layers": cfg.num_layers, "read_bytes": read}
                for n_dst in (1, 4):
                    dst = list(range(1, 1 + n_dst))
                    for _ in range(3):
                        gen.fork_session(0, dst)
                    us = stats([timed(lambda: gen.fork_session(0, dst)) for _ in range(args.repeats)])
                    moved = read * (1 + n_dst)
                    line[f"fork_{n_dst}"] = dict(us, written_bytes=read * n_dst, tb_per_s=moved / us["median_us"] / 1e6,
                                                 of_read_sol=moved / us["median_us"] / 1e6 / SOL_READ_TBS)
                a, b = torch.empty(read, dtype=torch.uint8, device=dev), torch.empty(read, dtype=torch.uint8, device=dev)
                for _ in range(3):
                    b.copy_(a)
                us = stats([timed(lambda: b.copy_(a)) for _ in range(args.repeats)])
                line["plain_d2d_copy"] = dict(us, tb_per_s=2 * read / us["median_us"] / 1e6)
                del a, b
                if not args.no_prefill:
                    T = valid
                    codes = torch.randint(0, cfg.card, (1, n_user, T), generator=g).to(dev)
                    toks = torch.cat([torch.randint(0, cfg.text_card, (1, 1, T), generator=g),
                                      torch.randint(0, cfg.card, (1, cfg.dep_q, T), generator=g)], 1).to(dev)
                    mask = torch.zeros(B, dtype=torch.bool, device=dev)
                    mask[1] = True
                    us = []
                    for _ in range(2):                                     # the first fill warms up
                        gen.reset_streaming(mask)
                        us.append(timed(lambda: gen.prefill(codes, toks, sessions=[1])))
                    line["prefill_same_frames"] = {"us": us[1], "warmup_us": us[0], "frames": T,
                                                   "times_the_fork_to_1": us[1] / line["fork_1"]["median_us"]}
                print(json.dumps(line), flush=True)
                lines.append(line)
        del gen, lm
        torch.cuda.empty_cache()
    print(json.dumps({"summary": [{"ring": l["ring"], "depth": l["depth"], "fork_1_us": l["fork_1"]["median_us"], "fork_4_us": l["fork_4"]["median_us"],
                                   "fork_1_tb_per_s": l["fork_1"]["tb_per_s"], "fork_4_tb_per_s": l["fork_4"]["tb_per_s"],
                                   "d2d_tb_per_s": l["plain_d2d_copy"]["tb_per_s"],
                                   "prefill_us": l.get("prefill_same_frames", {}).get("us")} for l in lines],
                      "device": torch.cuda.get_device_name(0), "read_sol_tb_per_s": SOL_READ_TBS}), flush=True)


if __name__ == "__main__":
    main()
