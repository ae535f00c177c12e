"""Golden vectors for the TTS script machine on the device, produced by RUNNING THE REFERENCE (build container only, with the
reference's `moshi` package importable: `PYTHONPATH=<reference>/moshi python tests/golden/make_golden_tts_machine.py`).
`moshi.models.tts` imports `sphn`, which the build container does not have; an empty stub module stands in for it
(`StateMachine` never touches it).

tts_machine.npz - the reference's `StateMachine.process` alone, no model: for `second_stream_ahead` 0 (prefix `a0_`) and 2 (`a2_`),
max_padding 3, initial_padding 2, TokenIds(card=97), every script of SCRIPTS driven by the crafted stream of sampled tokens
`sampled` [S].  Per script i: `s<i>_tokens`, `s<i>_first`, `s<i>_padding` (the flat script), `<p>s<i>_out` [S] (the output token
per step), `<p>s<i>_end` (end_step, -1 = None) and `<p>s<i>_times` (consumption_times).  The generator asserts that the streams
hold every situation listed in EVENTS; tests/tts_machine_cases.py re-derives them from the arrays.

lm_tts_machine.npz - the reference's `LMGen` on the tiny TTS model (moshi_amd.config.tiny_tts_config, the weights, conditions and
guidance of lm_tts.npz's scenario g: cfg_coef 2, cfg_is_no_text, cross + sum conditions, greedy), B = 3, driven by three hooks
that do what the closures of `TTSModel.generate` do (tts.py:553-583).  `TTSModel.generate` itself cannot be used: it asserts a
`condition_provider` and derives the condition tensors from speaker attributes, which needs conditioner modules and files.  The
hooks here are GLUE OF OUR OWN around the reference's `StateMachine.new_state` / `process` and `_delayed`: padding bonus 1.5,
delay_steps 2, second_stream_ahead 2, max_padding 3, initial_padding 2; session 1 has a text + audio prefix of 3 columns; the
depformer runs on every step (no `depformer_replace_tokens`).  Recorded as in lm_tts.npz (ring output, the logits every token was
sampled from - the text logits AFTER the bonus -, the sampled tokens), plus `text_out` (the machine's token), `pad_pre` (the pad
logit before the bonus), `end_steps`, `times<b>` and the scripts.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent

NEW_WORD, PAD, CARD = 0, 3, 97
MAX_PADDING, INITIAL_PADDING = 3, 2

# (tokens, padding) per entry.  0: 4-token words, then 1-token words, a break, a padded word.  1: the empty script.  2: a
# padded first word, a break in the middle, the script running out early
SCRIPTS = [
    [([10, 11, 12, 13], 0), ([20, 21, 22, 23], 0), ([30, 31, 32, 33], 0), ([40], 0), ([41], 0), ([], 2), ([50, 51], 1), ([60], 0)],
    [],
    [([70], 3), ([71, 72, 73], 0), ([], 1), ([80, 81], 0)],
]
# the sampled stream: new_word as early as allowed (words taken back to back: the lookahead queue fills up), tokens outside
# {new_word, pad}, then pads only (remaining_padding runs out and forces the words) until every script has run out
SAMPLED = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0, 3, 95, 0, 0] + [3] * 30
EVENTS = ("other_token", "break_entry", "forced_word", "two_words_in_lookahead", "end_step", "end_new_word_on_second", "empty_script")


def flat(script):
    toks, first, pads = [], [0], []
    for t, p in script:
        toks += t
        first.append(len(toks))
        pads.append(p)
    return np.array(toks, np.int32), np.array(first, np.int32), np.array(pads, np.int32)


def machine_golden(tts):
    out = {"sampled": np.array(SAMPLED, np.int32), "params": np.array([CARD, NEW_WORD, PAD, MAX_PADDING, INITIAL_PADDING], np.int32)}
    seen = set()
    for i, script in enumerate(SCRIPTS):
        out[f"s{i}_tokens"], out[f"s{i}_first"], out[f"s{i}_padding"] = flat(script)
        if not script:
            seen.add("empty_script")
    for ahead in (0, 2):
        m = tts.StateMachine(tts.TokenIds(card=CARD, new_word=NEW_WORD, pad=PAD), second_stream_ahead=ahead,
                             max_padding=MAX_PADDING, initial_padding=INITIAL_PADDING)
        for i, script in enumerate(SCRIPTS):
            state = m.new_state([tts.Entry(tokens=list(t), text="w", padding=p) for t, p in script])
            outs = []
            for step, tok in enumerate(SAMPLED):
                if tok not in (NEW_WORD, PAD):
                    seen.add("other_token")
                free = not state.queued and state.forced_padding <= 0
                if free and state.remaining_padding <= 0 and tok != NEW_WORD and state.entries:
                    seen.add("forced_word")
                n_before, la_before, end_before = len(state.entries), len(state.lookahead_queued), state.end_step
                o, consumed = m.process(step, state, tok)
                if consumed and not script[len(script) - n_before][0]:
                    seen.add("break_entry")
                if consumed and la_before > 0 and len(state.lookahead_queued) > la_before:
                    seen.add("two_words_in_lookahead")
                if end_before is None and state.end_step is not None:
                    seen.add("end_step")
                    if ahead and o // CARD - 1 == NEW_WORD:
                        seen.add("end_new_word_on_second")
                outs.append(o)
            assert state.end_step is not None, "the stream must run every script out"
            out[f"a{ahead}_s{i}_out"] = np.array(outs, np.int32)
            out[f"a{ahead}_s{i}_end"] = np.array([state.end_step], np.int32)
            out[f"a{ahead}_s{i}_times"] = np.array(state.consumption_times, np.int32)
    assert seen == set(EVENTS), f"missing situations: {set(EVENTS) - seen}"
    np.savez_compressed(HERE / "tts_machine.npz", **out)
    print("tts_machine.npz", {k: v.shape for k, v in out.items()})


LM_SCRIPTS = [
    [([10, 11], 0), ([20], 1), ([], 1), ([30, 31, 32], 0), ([40], 0)],
    [([50], 0), ([51, 52], 0), ([53], 0)],
    [([60, 61, 62], 0), ([70], 0)],
]


def lm_golden(tts):
    import moshi.models.lm as lm_mod
    from moshi.conditioners.base import ConditionFuser, ConditionType
    from moshi_amd.config import tiny_tts_config
    from moshi_amd.weights import random_lm_state_dict
    B, S, BONUS, DELAY_STEPS, AHEAD = 3, 16, 1.5, 2, 2
    cfg = tiny_tts_config()
    seed = 61
    sd = random_lm_state_dict(cfg, seed=seed)
    lm = lm_mod.LMModel(**cfg.reference_kwargs(), fuser=ConditionFuser({"sum": ["s"], "cross": ["x"]}), device="cpu", dtype=torch.bfloat16)
    lm.load_state_dict(dict(sd), strict=True)
    lm.eval()
    g = torch.Generator().manual_seed(23)
    cross = (0.7 * torch.randn(2 * B, 4, cfg.dim, generator=g)).to(torch.bfloat16)
    sums = (0.5 * torch.randn(2 * B, 1, cfg.dim, generator=g)).to(torch.bfloat16)
    T = 3
    prefix = torch.randint(0, cfg.card, (cfg.n_q + 1, T), generator=g)
    prefix[0] = torch.tensor([5, (17 + 1) * CARD + 6, 7])            # a plain, a muxed and a plain text token
    ct = lambda t: ConditionType(t, torch.ones(t.shape[:2], dtype=torch.bool))

    ids = tts.TokenIds(card=CARD, new_word=NEW_WORD, pad=PAD)
    machine = tts.StateMachine(ids, second_stream_ahead=AHEAD, max_padding=MAX_PADDING, initial_padding=INITIAL_PADDING)
    states = [machine.new_state([tts.Entry(tokens=list(t), text="w", padding=p) for t, p in sc]) for sc in LM_SCRIPTS]
    text_prefix = {1: prefix[0].tolist()}
    delays = [d + DELAY_STEPS for d in lm.delays[lm.audio_offset:]]
    audio_prefix = {1: tts._delayed(prefix[lm.audio_offset:], delays, ids.ungenerated)}
    cur = {"step": 0}
    rec = {"pad_pre": [], "text_out": []}

    def on_text_logits(logits):
        rec["pad_pre"].append(logits[:B, 0, 0, ids.pad].float().numpy().copy())
        logits[..., ids.pad] += BONUS

    def on_text(tokens):
        step, outs = cur["step"], []
        for b, tok in enumerate(tokens.tolist()):
            if b in text_prefix and step < len(text_prefix[b]):
                outs.append(text_prefix[b][step])
            else:
                outs.append(machine.process(step, states[b], tok)[0])
        rec["text_out"].append(np.array(outs, np.int64))
        tokens[:] = torch.tensor(outs, dtype=torch.long)

    def on_audio(audio):
        step = cur["step"]
        for q in range(audio.shape[1]):
            if step < delays[q]:
                audio[:, q] = ids.zero
        for b, pre in audio_prefix.items():
            if step < pre.shape[1]:
                col = pre[:, step]
                audio[b] = torch.where(col != ids.ungenerated, col, audio[b])

    gen = lm_mod.LMGen(lm, use_sampling=False, support_out_of_sync=True, cfg_coef=2.0, cfg_is_no_text=True,
                       condition_tensors={"s": ct(sums), "x": ct(cross)}, on_text_logits_hook=on_text_logits, on_text_hook=on_text,
                       on_audio_hook=on_audio)
    out = {"tokens": [], "text_logits": [], "audio_logits": [], "text_tok": [], "audio_tok": []}
    calls = []
    orig = lm_mod.sample_token

    def sample_token(logits, *a, **k):
        tok = orig(logits, *a, **k)
        calls.append((logits.float().numpy().reshape(logits.shape[0], -1).copy(), tok.numpy().reshape(-1).copy()))
        return tok
    lm_mod.sample_token = sample_token
    try:
        with torch.no_grad(), gen.streaming(B):
            for s in range(S):
                cur["step"] = s
                calls.clear()
                o = gen.step(torch.zeros(B, 0, 1, dtype=torch.long))
                out["tokens"].append(o.numpy().copy())
                out["text_logits"].append(calls[0][0]); out["text_tok"].append(calls[0][1])
                out["audio_logits"].append(np.stack([c[0] for c in calls[1:]], 1))
                out["audio_tok"].append(np.stack([c[1] for c in calls[1:]], 1))
    finally:
        lm_mod.sample_token = orig
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(seed=np.array([seed]), cross=cross.float().numpy(), sum=sums.float().numpy(), prefix=prefix.numpy(),
               pad_pre=np.stack(rec["pad_pre"]), text_out=np.stack(rec["text_out"]),
               params=np.array([CARD, NEW_WORD, PAD, MAX_PADDING, INITIAL_PADDING, AHEAD, DELAY_STEPS], np.int32), bonus=np.array([BONUS], np.float32),
               end_steps=np.array([-1 if st.end_step is None else st.end_step for st in states], np.int32))
    for b, sc in enumerate(LM_SCRIPTS):
        res[f"s{b}_tokens"], res[f"s{b}_first"], res[f"s{b}_padding"] = flat(sc)
        res[f"times{b}"] = np.array(states[b].consumption_times, np.int32)
    # the bonus is added in the logits' own dtype: bf16(float(l) + bonus)
    want = (torch.from_numpy(res["pad_pre"]) + BONUS).to(torch.bfloat16).float().numpy()
    assert np.array_equal(want, res["text_logits"][:, :, PAD]), "the reference does not add the bonus as bf16(float(l) + bonus)"
    assert (res["text_out"] != res["text_tok"]).any() and (res["end_steps"] >= 0).any()
    np.savez_compressed(HERE / "lm_tts_machine.npz", **res)
    print("lm_tts_machine.npz", {k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent.parent))
    sys.modules.setdefault("sphn", types.ModuleType("sphn"))
    from moshi.models import tts as tts_mod
    machine_golden(tts_mod)
    lm_golden(tts_mod)
