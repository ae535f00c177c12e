"""Step time of a TTS-family LM (kyutai's TTS checkpoints: n_q = dep_q = 32, depformer weight schedule, low-rank depformer
embeddings, demuxed text stream, cross-attention) on the engine.

    python scripts/bench_tts_lm.py [--batches 1,8,32] [--steps 200] [--warmup 20] [--machine none|host|device]

The model has the 1.6B shape modelled on the published TTS configuration (dim 2048 x 16 layers, depformer 1024 x 4 layers, 32
micro-steps over 9 weight sets, rank 128) with seeded random weights: nothing is downloaded and the exact published values
are not verified here.  ms per `LMGen.step` from device events over `--steps` steps after `--warmup`, sampling on, one
16-position `cross` condition.  Prints ONE JSON line; frames/s = B * 1000 / ms against the 12.5 Hz real-time rate.

--machine: the TTS script machine around the step (every session runs a seeded script of 400 words of 1-4 tokens; lookahead 2,
max_padding 8, initial_padding 2, delay_steps 16).  `none`: the bare step, as before.  `host`: three Python hooks doing what the
closures of the reference's `TTSModel.generate` do - `.tolist()` of the text tokens, the machine per row in Python, the token
written back, the delayed codebooks zeroed - so the step runs in eager segments.  `device`: `LMGen(tts_machine=...)`, the same
machine inside the captured step.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def tts_16b_config():
    from moshi_amd.config import LMConfig
    return LMConfig(dim=2048, num_heads=16, num_layers=16, hidden_scale=4.125, context=500, n_q=32, dep_q=32, card=2048, text_card=8000,
                    depformer_dim=1024, depformer_dim_feedforward=int(4.125 * 1024), depformer_num_heads=16, depformer_num_layers=4,
                    delays=[0] + [2] * 32, cross_attention=True, depformer_weights_per_step_schedule=list(range(8)) + [8] * 24,
                    depformer_low_rank_embeddings=128, demux_second_text_stream=True)


class HostMachine:
    """One session's script machine on the host, for --machine host."""

    def __init__(self, entries, m):
        from collections import deque
        self.entries, self.m = deque(entries), m
        self.remaining = self.forced = m.initial_padding
        self.queued, self.look, self.end_step = deque(), deque(), None

    def process(self, step, token):
        m = self.m
        if token not in (m.new_word, m.pad) or self.queued or self.forced > 0:
            token = m.pad
        elif self.remaining <= 0:
            token = m.new_word
        if token == m.new_word:
            if self.entries:
                toks, padding = self.entries.popleft()
                if toks:
                    self.queued.extend(toks)
                    ahead = m.second_stream_ahead
                    for t, _ in self.entries if ahead else ():
                        if t:
                            ahead -= 1
                            if ahead == 0:
                                self.look.extend(t)
                                break
                    self.remaining = m.max_padding
                else:
                    token = m.pad
                self.forced = padding
            else:
                token = m.new_word if m.second_stream_ahead and self.end_step is None else m.pad
                if self.end_step is None:
                    self.end_step = step
        if token == m.pad:
            self.remaining -= self.remaining > 0
            self.forced -= self.forced > 0
            out = self.queued.popleft() if self.queued else m.pad
        else:
            out = m.new_word
        if m.second_stream_ahead:
            second = -1
            if out == m.new_word:
                second = m.new_word
                out = self.queued.popleft() if self.queued else m.pad
            elif self.look:
                second = self.look.popleft()
            out = (second + 1) * m.text_card + out
        return out


def make_scripts(B, cfg, words=400):
    g = torch.Generator().manual_seed(2)
    scripts = []
    for _ in range(B):
        lens = torch.randint(1, 5, (words,), generator=g).tolist()
        scripts.append([(torch.randint(4, cfg.text_card, (n,), generator=g).tolist(), 0) for n in lens])
    return scripts


def host_hooks(cfg, m, scripts):
    machines = [HostMachine(sc, m) for sc in scripts]
    delays = [d + m.delay_steps for d in cfg.delays[1:]]
    step = {"s": 0}

    def on_text_logits(t):
        if m.padding_bonus:
            t[..., m.pad] += m.padding_bonus

    def on_text(t):
        out = [mach.process(step["s"], tok) for mach, tok in zip(machines, t.tolist())]
        t[:] = torch.tensor(out, dtype=torch.long, device=t.device)

    def on_audio(t):
        for q, d in enumerate(delays):
            if step["s"] < d:
                t[:, q] = m.zero
        step["s"] += 1
    return dict(on_text_logits_hook=on_text_logits, on_text_hook=on_text, on_audio_hook=on_audio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--machine", choices=["none", "host", "device"], default="none")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from moshi_amd.lm import ConditionFuser, LMGen, LMModel
    if args.machine != "none":
        from moshi_amd.lm import TTSMachine, TTSScript
    from moshi_amd.weights import random_lm_state_dict
    cfg = tts_16b_config()
    sd = random_lm_state_dict(cfg, seed=0, device="cuda")
    n_params = sum(v.numel() for v in sd.values())
    res = {"metric": "tts_lm_step_ms", "model": "tts-1.6b-shape (random init)", "params": n_params, "steps": args.steps,
           "warmup": args.warmup, "frame_rate_hz": 12.5, "machine": args.machine, "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        lm = LMModel(sd, cfg, device="cuda", max_batch=B, fuser=ConditionFuser({"cross": ["x"]}))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = (0.5 * torch.randn(B, 16, cfg.dim, generator=g, device="cuda")).to(torch.bfloat16)
        kw = {}
        if args.machine != "none":
            m = TTSMachine(text_card=cfg.text_card + 1, second_stream_ahead=2, max_padding=8, initial_padding=2, delay_steps=16,
                           max_entries=400, max_tokens=1600)
            scripts = make_scripts(B, cfg)
            kw = host_hooks(cfg, m, scripts) if args.machine == "host" else {"tts_machine": m}
        gen = LMGen(lm, use_sampling=True, condition_tensors={"x": (x, torch.ones(B, 16, dtype=torch.bool, device="cuda"))}, **kw)
        codes = torch.zeros(B, 0, 1, dtype=torch.int64, device="cuda")
        with gen.streaming(B):
            if args.machine == "device":
                for b, sc in enumerate(scripts):
                    gen.set_session_script(b, TTSScript(entries=sc))
            for _ in range(args.warmup):
                gen.step(codes)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                gen.step(codes)
            t1.record()
            torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.steps
        res["batches"][str(B)] = {"ms_per_step": round(ms, 4), "frames_per_s": round(B * 1000.0 / ms, 1),
                                  "x_real_time": round(1000.0 / ms / 12.5, 1)}
        del gen, lm
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
