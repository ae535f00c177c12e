"""Shared checks of the TTS script machine on the device (mmi_lm_enable_tts_machine) against the reference's
`StateMachine` (tests/golden/tts_machine.npz) and the reference's `LMGen` driven by generate()-style hooks
(tests/golden/lm_tts_machine.npz) - run on the kernel simulator and on the GPU.  `HostMachine` restates the machine in Python for
the device-against-host comparison; it is held to the golden itself."""
from __future__ import annotations

import os
from collections import deque
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from moshi_amd.config import tiny_tts_config
from moshi_amd.lm import ConditionFuser, LMGen, LMModel, TTSMachine, TTSScript
from moshi_amd.weights import random_lm_state_dict
from tests.lm_cases import GUIDED_WIDEN, logits_close
from tests.tts_cases import h_config

GOLDEN = Path(__file__).resolve().parent / "golden"
EVENTS = {"other_token", "break_entry", "forced_word", "two_words_in_lookahead", "end_step", "end_new_word_on_second", "empty_script"}


@lru_cache(maxsize=None)
def golden(name):
    return dict(np.load(GOLDEN / name))


def entries_of(g, i):
    toks, first, pads = g[f"s{i}_tokens"], g[f"s{i}_first"], g[f"s{i}_padding"]
    return [(toks[first[e]:first[e + 1]].tolist(), int(pads[e])) for e in range(len(pads))]


class HostMachine:
    """The machine restated on the host: one session's state, `process(step, token)` -> output token, and the situations met."""

    def __init__(self, entries, card, new_word, pad, ahead, max_padding, initial_padding):
        self.entries = deque(entries)
        self.card, self.new_word, self.pad, self.ahead, self.max_padding = card, new_word, pad, ahead, max_padding
        self.remaining = self.forced = initial_padding
        self.queued, self.look = deque(), deque()
        self.end_step, self.times, self.seen = None, [], set()
        if not entries:
            self.seen.add("empty_script")

    def process(self, step, token):
        if token not in (self.new_word, self.pad):
            self.seen.add("other_token")
            token = self.pad
        if self.queued or self.forced > 0:
            token = self.pad
        elif self.remaining <= 0:
            if token != self.new_word and self.entries:
                self.seen.add("forced_word")
            token = self.new_word
        ended_now = False
        if token == self.new_word:
            if self.entries:
                toks, padding = self.entries.popleft()
                self.times.append(step)
                if toks:
                    self.queued.extend(toks)
                    if self.ahead:
                        left = [t for t, _ in self.entries if t]
                        if len(left) >= self.ahead:
                            if self.look:
                                self.seen.add("two_words_in_lookahead")
                            self.look.extend(left[self.ahead - 1])
                    self.remaining = self.max_padding
                else:
                    self.seen.add("break_entry")
                    token = self.pad
                self.forced = padding
            else:
                token = self.pad
                if self.end_step is None:
                    self.end_step, ended_now = step, True
                    self.seen.add("end_step")
                    if self.ahead:
                        token = self.new_word
        if token == self.pad:
            self.remaining -= self.remaining > 0
            self.forced -= self.forced > 0
            out = self.queued.popleft() if self.queued else self.pad
        else:
            out = self.new_word
        if self.ahead:
            second = -1
            if out == self.new_word:
                second = self.new_word
                if ended_now:
                    self.seen.add("end_new_word_on_second")
                out = self.queued.popleft() if self.queued else self.pad
            elif self.look:
                second = self.look.popleft()
            out = (second + 1) * self.card + out
        return out


def check_golden_holds_every_situation_and_host_machine_equals_it():
    """tts_machine.npz re-read: the host restatement reproduces every recorded stream, and the streams hold every situation the
    generator asserted."""
    g = golden("tts_machine.npz")
    card, new_word, pad, max_padding, initial_padding = (int(v) for v in g["params"])
    seen = set()
    for ahead in (0, 2):
        for i in range(3):
            m = HostMachine(entries_of(g, i), card, new_word, pad, ahead, max_padding, initial_padding)
            outs = [m.process(s, int(t)) for s, t in enumerate(g["sampled"])]
            assert outs == g[f"a{ahead}_s{i}_out"].tolist(), (ahead, i)
            assert m.end_step == int(g[f"a{ahead}_s{i}_end"][0]) and m.times == g[f"a{ahead}_s{i}_times"].tolist()
            seen |= m.seen
    assert seen == EVENTS, EVENTS - seen


# ---- models -------------------------------------------------------------------------------------------------------------------
def machine_of(params, ahead, **kw):
    card, new_word, pad, max_padding, initial_padding = (int(v) for v in params[:5])
    return TTSMachine(text_card=card, new_word=new_word, pad=pad, second_stream_ahead=ahead, max_padding=max_padding,
                      initial_padding=initial_padding, max_entries=kw.pop("max_entries", 8), max_tokens=kw.pop("max_tokens", 20), **kw)


_MODELS = {}


def model(device, lib, kind, no_graph=False):
    """`tts`: tiny_tts_config with the weights of lm_tts_machine.npz (demuxed text, 6 model rows for 3 guided sessions);
    `h`: tests.tts_cases.h_config (no demux, grouped depformer_in).  Cached per library: the checks only stream on them."""
    key = (str(device), id(lib), kind, no_graph)
    if key not in _MODELS:
        if kind == "tts":
            cfg, seed, fuser, rows = tiny_tts_config(), int(golden("lm_tts_machine.npz")["seed"][0]), ConditionFuser({"sum": ["s"], "cross": ["x"]}), 6
        else:
            cfg, seed, fuser, rows = h_config(), 67, None, 3
        old = os.environ.get("MMI_NO_GRAPH")
        if no_graph:
            os.environ["MMI_NO_GRAPH"] = "1"
        try:
            _MODELS[key] = LMModel(random_lm_state_dict(cfg, seed=seed), cfg, device=device, max_batch=rows, lib=lib, fuser=fuser)
        finally:
            if no_graph:
                os.environ.pop("MMI_NO_GRAPH") if old is None else os.environ.__setitem__("MMI_NO_GRAPH", old)
    return _MODELS[key]


def tts_gen(device, lib, machine, no_graph=False, **kw):
    g = golden("lm_tts_machine.npz")
    t = lambda k: torch.from_numpy(g[k]).to(torch.bfloat16)
    conds = {"s": (t("sum"), torch.ones(6, 1, dtype=torch.bool)), "x": (t("cross"), torch.ones(6, 4, dtype=torch.bool))}
    kw.setdefault("use_sampling", False)
    return LMGen(model(device, lib, "tts", no_graph), support_out_of_sync=True, cfg_coef=2.0, cfg_is_no_text=True, condition_tensors=conds,
                 tts_machine=machine, **kw)


def codes_for(gen, B):
    cfg = gen.lm_model.config
    return torch.zeros(B, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device=gen.device)


def text_lag(gen):
    """Steps between a text token entering the ring and leaving it in the output frame."""
    d = list(gen.lm_model.delays)
    return max(d) - d[0]


def run(gen, B, steps, scripts=None, forced_text=None, taps=False, before_step=None):
    """Streams `steps` frames; returns the ring outputs [steps, B, 1 + dep_q] (and the taps), leaving the stream open for the
    caller's `finish`.  scripts: {session: TTSScript}; forced_text [steps] or [steps, B]: the sampled text token of every step."""
    dep_q = gen.lm_model.dep_q
    gen.streaming_forever(B)
    for b, sc in (scripts or {}).items():
        gen.set_session_script(b, sc)
    outs, tls = [], []
    for s in range(steps):
        if before_step is not None:
            before_step(s)
        forced = None
        if forced_text is not None and s < len(forced_text):
            forced = torch.full((B, 1 + dep_q), -1, dtype=torch.int64)
            forced[:, 0] = torch.as_tensor(forced_text[s])
        out, tl, _ = gen.step_with_taps(codes_for(gen, B), forced_tokens=forced) if taps or forced is not None else (gen.step(codes_for(gen, B)), None, None)
        outs.append(out.cpu().numpy()[:, :, 0])
        if taps:
            tls.append(tl.cpu().numpy())
    return np.stack(outs), tls


# ---- 1. the machine alone ---------------------------------------------------------------------------------------------------------
def check_machine_alone(device, lib, ahead):
    """The sampled text tokens of tts_machine.npz forced through `forced_tokens`: the engine's text token per step, end_step,
    n_consumed and consumption_times equal the reference's, for every script; a session without a script passes its token
    through.  second_stream_ahead 0 runs on the model without a demuxed text stream, 2 on the demuxed one."""
    g = golden("tts_machine.npz")
    S = len(g["sampled"])
    for layout in ((0, 2, None), (1, None, 0)):
        m = machine_of(g["params"], ahead)
        gen = tts_gen(device, lib, m) if ahead else LMGen(model(device, lib, "h"), use_sampling=False, support_out_of_sync=True, tts_machine=m)
        lag = text_lag(gen)
        scripts = {b: TTSScript(entries=entries_of(g, i)) for b, i in enumerate(layout) if i is not None}
        status = {}

        def grab(s):
            if s == S:
                status.update({b: gen.session_script_status(b) for b in range(3)})
        try:
            outs, _ = run(gen, 3, S + lag, scripts, forced_text=g["sampled"], before_step=grab)
        finally:
            gen._stop_streaming()
        for b, i in enumerate(layout):
            got = outs[lag:, b, 0]
            if i is None:
                assert np.array_equal(got, g["sampled"]), f"session {b} has no script: its tokens must pass through"
                assert not status[b].has_script and status[b].n_consumed == 0 and status[b].end_step is None
                continue
            assert np.array_equal(got, g[f"a{ahead}_s{i}_out"]), f"ahead {ahead} script {i}: text tokens differ\n{got}\n{g[f'a{ahead}_s{i}_out']}"
            assert status[b].end_step == int(g[f"a{ahead}_s{i}_end"][0])
            assert status[b].consumption_times == g[f"a{ahead}_s{i}_times"].tolist() and status[b].n_consumed == len(g[f"a{ahead}_s{i}_times"])


# ---- 2. the whole step against the reference -----------------------------------------------------------------------------------
def lm_machine(g, bonus=None, **kw):
    ahead, delay_steps = int(g["params"][5]), int(g["params"][6])
    return machine_of(g["params"], ahead, delay_steps=delay_steps, padding_bonus=float(g["bonus"][0]) if bonus is None else bonus,
                      max_prefix=3, **kw)


def lm_scripts(g):
    sc = {b: TTSScript(entries=entries_of(g, b)) for b in range(3)}
    sc[1].text_prefix = g["prefix"][0].tolist()
    sc[1].audio_prefix = g["prefix"][1:]
    return sc


def _bf16_add(x, bonus):
    return (torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float() + bonus).to(torch.bfloat16).float().numpy()


def check_whole_step_against_reference(device, lib):
    """lm_tts_machine.npz replayed teacher-forced with the machine on the device and no host hook: ring outputs identical, logits
    within the tolerances of tests/tts_cases.py, the script status the reference's; and against the same replay without the
    bonus: the pad logit is bf16(l + bonus) bit for bit, every other text logit untouched."""
    g = golden("lm_tts_machine.npz")
    S, B = g["text_tok"].shape
    dep_q = g["audio_tok"].shape[2]
    taps = {}
    for bonus in (None, 0.0):
        gen = tts_gen(device, lib, lm_machine(g, bonus))
        gen.streaming_forever(B)
        try:
            for b, sc in lm_scripts(g).items():
                gen.set_session_script(b, sc)
            tls = []
            for s in range(S):
                forced = np.concatenate([g["text_tok"][s][:, None], g["audio_tok"][s]], 1)
                out, tl, al = gen.step_with_taps(codes_for(gen, B), forced_tokens=torch.from_numpy(forced))
                out, tl, al = out.cpu().numpy(), tl.cpu().numpy(), al.cpu().numpy()
                tls.append(tl)
                assert np.array_equal(out, g["tokens"][s]), f"step {s}: ring output differs (bonus {bonus})"
                if bonus is None:
                    for b in range(B):
                        assert logits_close(tl[b], g["text_logits"][s, b]), f"step {s} row {b}: text logits"
                        for k in range(dep_q):
                            assert logits_close(al[b, k], g["audio_logits"][s, b, k], GUIDED_WIDEN), f"step {s} row {b} cb {k}: audio logits"
            taps[bonus] = np.stack(tls)
            for b in range(B):
                st = gen.session_script_status(b)
                assert (-1 if st.end_step is None else st.end_step) == int(g["end_steps"][b]) and st.consumption_times == g[f"times{b}"].tolist()
        finally:
            gen._stop_streaming()
    pad, bonus = int(g["params"][2]), float(g["bonus"][0])
    on, off = taps[None], taps[0.0]
    assert np.array_equal(on[:, :, pad], _bf16_add(off[:, :, pad], bonus)), "the pad logit is not bf16(l + bonus)"
    assert not np.array_equal(on[:, :, pad], off[:, :, pad])
    rest = np.arange(on.shape[2]) != pad
    assert np.array_equal(on[:, :, rest], off[:, :, rest]), "the bonus touched another logit"
    # the reference's own arithmetic, from its recorded pre-bonus logit
    assert np.array_equal(_bf16_add(g["pad_pre"], bonus), g["text_logits"][:, :, pad])


# ---- 3. device against host ---------------------------------------------------------------------------------------------------------
def host_hooks(gen_cfg, g, m, scripts, B):
    """Python hooks doing what the device machine does (the closures of TTSModel.generate around HostMachine)."""
    delays = [d + m.delay_steps for d in list(gen_cfg.delays)[1:]]
    machines = {b: HostMachine(sc.entries, m.text_card, m.new_word, m.pad, m.second_stream_ahead, m.max_padding, m.initial_padding)
                for b, sc in scripts.items()}
    step = {"s": 0}

    def on_logits(t):
        if m.padding_bonus:
            t[..., m.pad] += m.padding_bonus

    def on_text(t):
        toks = t.tolist()
        for b, mach in machines.items():
            tp = scripts[b].text_prefix
            toks[b] = tp[step["s"]] if tp is not None and step["s"] < len(tp) else mach.process(step["s"], toks[b])
        t.copy_(torch.tensor(toks, dtype=torch.long))

    def on_audio(t):
        s = step["s"]
        for q, d in enumerate(delays):
            if s < d:
                t[:, q] = m.zero
            for b, sc in scripts.items():
                if sc.audio_prefix is not None and 0 <= s - d < len(sc.audio_prefix[q]) and int(sc.audio_prefix[q][s - d]) != -2:
                    t[b, q] = int(sc.audio_prefix[q][s - d])
    return dict(on_text_logits_hook=on_logits, on_text_hook=on_text, on_audio_hook=on_audio), step, machines


def check_device_equals_host(device, lib, steps=16):
    """The same free-running stream with seeded sampling, once with the machine on the device and once with Python hooks that
    restate it: identical tokens step for step, and the same script status."""
    g = golden("lm_tts_machine.npz")
    m, scripts = lm_machine(g), lm_scripts(g)
    gen = tts_gen(device, lib, m, use_sampling=True, seed=11)
    try:
        dev_out, _ = run(gen, 3, steps, scripts)
        dev_status = [gen.session_script_status(b) for b in range(3)]
    finally:
        gen._stop_streaming()
    hooks, step, machines = host_hooks(gen.lm_model.config, g, m, scripts, 3)
    gen = tts_gen(device, lib, None, use_sampling=True, seed=11, **hooks)
    try:
        host_out, _ = run(gen, 3, steps, before_step=lambda s: step.update(s=s))
    finally:
        gen._stop_streaming()
    assert np.array_equal(dev_out, host_out), f"first difference at step {int(np.argwhere((dev_out != host_out).any((1, 2)))[0])}"
    for b in range(3):
        assert dev_status[b].end_step == machines[b].end_step and dev_status[b].consumption_times == machines[b].times
    assert any(st.n_consumed > 0 for st in dev_status)


def check_host_hooks_run_behind_the_machine(device, lib, steps=6):
    """Host hooks next to the machine see its tokens and what they write is what the step continues with."""
    g = golden("lm_tts_machine.npz")
    m, scripts = lm_machine(g), lm_scripts(g)
    seen = {"text": [], "audio": []}

    def on_text(t):
        seen["text"].append(t.cpu().numpy().copy())
        t[2] = 9

    def on_audio(t):
        seen["audio"].append(t.cpu().numpy().copy())
        t[0, 0] = 5
    gen = tts_gen(device, lib, m, on_text_hook=on_text, on_audio_hook=on_audio)
    ref = tts_gen(device, lib, m)
    try:
        out, _ = run(gen, 3, steps, scripts, forced_text=g["text_tok"])
    finally:
        gen._stop_streaming()
    try:
        want, _ = run(ref, 3, steps, scripts, forced_text=g["text_tok"])
    finally:
        ref._stop_streaming()
    text = np.stack(seen["text"])
    assert np.array_equal(text, g["text_out"][:steps]), "on_text_hook did not see the machine's tokens"
    audio = np.stack(seen["audio"])
    assert (audio[0] == -1).all() and (audio[1][:, :1] == -1).all(), "on_audio_hook did not see the zeroed codebooks"
    lag = text_lag(gen)
    assert (out[lag:, 2, 0] == 9).all() and np.array_equal(out[lag:, :2, 0], want[lag:, :2, 0])
    assert (out[lag:, 0, 1] == 5).all()


# ---- 4. lifecycle -------------------------------------------------------------------------------------------------------------
def check_lifecycle(device, lib):
    """Free-running greedy streams of the scripts of lm_tts_machine.npz against the undisturbed stream `base`."""
    g = golden("lm_tts_machine.npz")
    m, scripts = lm_machine(g), lm_scripts(g)
    B, S = 3, 16

    def stream(ops, steps=S):
        gen = tts_gen(device, lib, m)
        try:
            out, _ = run(gen, B, steps, scripts, before_step=lambda s: ops(gen, s))
            return out, [gen.session_script_status(b) for b in range(B)]
        finally:
            gen._stop_streaming()
    base, base_st = stream(lambda gen, s: None)
    assert all(st.n_consumed > 0 for st in base_st)

    # a row masked for two steps: its state and status do not move, and it continues where it stood
    mid = {}

    def masked(gen, s):
        if s == 5:
            mid["before"] = gen.session_script_status(1)
            gen.set_exec_mask(torch.tensor([True, False, True]))
        if s == 7:
            mid["after"] = gen.session_script_status(1)
            gen.set_exec_mask(torch.tensor([True, True, True]))
    out, st = stream(masked, S + 2)
    assert mid["before"] == mid["after"], "a masked row's machine moved"
    assert np.array_equal(out[:5, 1], base[:5, 1]) and np.array_equal(out[7:, 1], base[5:, 1]), "the masked row does not continue where it stood"
    assert np.array_equal(out[:S, 0], base[:, 0]) and st[1] == base_st[1]

    # reset of one row: that row starts over on the same script like a fresh stream, the others go on
    def reset(gen, s):
        if s == 6:
            gen.reset_streaming(torch.tensor([False, False, True]))
    out, st = stream(reset)
    assert np.array_equal(out[:, :2], base[:, :2]) and st[:2] == base_st[:2], "the reset touched another row"
    assert np.array_equal(out[6:, 2], base[:S - 6, 2]), "the reset row does not continue like a fresh stream"
    assert st[2].consumption_times == [t for t in base_st[2].consumption_times if t < S - 6]

    # save at step 10, run on, load at 13, run on again: the same continuation and status
    snap = {}

    def save_load(gen, s):
        if s == 10:
            snap["state"] = gen.get_streaming_state()
        if s == 13:
            gen.set_streaming_state(snap["state"])
    out, st = stream(save_load, S + 3)
    assert np.array_equal(out[:13], base[:13]) and np.array_equal(out[13:], base[10:]) and st == base_st

    # a new script for one row between two steps: the other rows' tokens do not change
    def swap(gen, s):
        if s == 4:
            gen.set_session_script(0, TTSScript(entries=[([33], 0)]))
    out, st = stream(swap)
    assert np.array_equal(out[:, 1:], base[:, 1:]) and not np.array_equal(out[:, 0], base[:, 0])
    assert st[0].consumption_times and st[0].consumption_times[0] >= 4 and st[1:] == base_st[1:]


# ---- 5. graph and launch list -----------------------------------------------------------------------------------------------------
def launch_lists(device, lib):
    """(never enabled, enabled and switched off again, on) for the demuxed model and for the model without a demuxed text stream."""
    g = golden("tts_machine.npz")
    res = {}
    for kind in ("tts", "h"):
        lists = []
        for how in ("never", "off", "on"):
            m = machine_of(g["params"], 2 if kind == "tts" else 0) if how == "on" else None
            if how == "off":            # a stream with the machine first: the next one without it must not keep anything of it
                check = tts_gen(device, lib, machine_of(g["params"], 0)) if kind == "tts" else LMGen(model(device, lib, kind), use_sampling=False, tts_machine=machine_of(g["params"], 0))
                check.streaming_forever(3)
                check._stop_streaming()
            gen = tts_gen(device, lib, m) if kind == "tts" else LMGen(model(device, lib, kind), use_sampling=False, support_out_of_sync=True, tts_machine=m)
            gen.streaming_forever(3)
            try:
                gen.step(codes_for(gen, 3))
                lists.append(gen.launch_list())
            finally:
                gen._stop_streaming()
        res[kind] = lists
    return res


def check_launch_budget(device, lib):
    ll = launch_lists(device, lib)
    for kind, extra in (("tts", 1), ("h", 2)):
        never, off, on = ll[kind]
        assert off == never, f"{kind}: a handle with the machine off does not build the launch list of one that never enabled it"
        assert len(on) <= len(never) + extra, f"{kind}: {len(on) - len(never)} launches more with the machine on (budget {extra})"
        assert any(k == "k_tts_machine" for _, k in on) and not any(k == "k_tts_machine" for _, k in never)
    assert not any(k == "k_dep_next_input_demux" for _, k in ll["tts"][2]), "the machine's launch replaces dep.in_demux"


def check_eager_equals_graphed(device, lib, steps=12):
    """The machine-on step run eagerly (MMI_NO_GRAPH at create) and as a captured graph: identical tokens and status."""
    g = golden("lm_tts_machine.npz")
    res = []
    for no_graph in (True, False):
        gen = tts_gen(device, lib, lm_machine(g), no_graph=no_graph, use_sampling=True, seed=5)
        try:
            out, _ = run(gen, 3, steps, lm_scripts(g))
            res.append((out, [gen.session_script_status(b) for b in range(3)]))
        finally:
            gen._stop_streaming()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def check_refusals(device, lib):
    from dataclasses import replace
    from moshi_amd.config import tiny_stt_config
    g = golden("lm_tts_machine.npz")
    good = lm_machine(g)
    # enabling
    stt = tiny_stt_config()
    if stt.dep_q == 0:
        lm0 = LMModel(random_lm_state_dict(stt, seed=37), stt, device=device, max_batch=2, lib=lib)
        with pytest.raises(NotImplementedError, match="dep_q"):
            LMGen(lm0, tts_machine=replace(good, second_stream_ahead=0)).streaming_forever(2)
    with pytest.raises(NotImplementedError, match="demuxed"):
        LMGen(model(device, lib, "h"), tts_machine=good).streaming_forever(2)
    # a stream without the machine: both calls are MMI_ERR_STATE
    gen = tts_gen(device, lib, None)
    gen.streaming_forever(3)
    try:
        with pytest.raises(RuntimeError, match="not enabled"):
            gen.set_session_script(0, TTSScript(entries=[([5], 0)]))
        with pytest.raises(RuntimeError, match="not enabled"):
            gen.session_script_status(0)
    finally:
        gen._stop_streaming()
    gen = tts_gen(device, lib, good)
    with pytest.raises(AssertionError):
        gen.set_session_script(0, TTSScript())                      # not streaming (LMGen's own assertion; the engine: MMI_ERR_STATE)
    st = _capi_status(gen, lib)
    assert st == -3, "mmi_lm_set_row_script outside a stream must return MMI_ERR_STATE"
    scripts = lm_scripts(g)
    gen.streaming_forever(3)
    try:
        for b, sc in scripts.items():
            gen.set_session_script(b, sc)
        for _ in range(3):
            gen.step(codes_for(gen, 3))
        before = [gen.session_script_status(b) for b in range(3)]
        bad = [
            (ValueError, "session", lambda: gen.set_session_script(3, scripts[0])),
            (ValueError, "session", lambda: gen.set_session_script(-1, None)),
            (ValueError, "vocabulary", lambda: gen.set_session_script(0, TTSScript(entries=[([5, 97], 0)]))),
            (ValueError, "vocabulary", lambda: gen.set_session_script(0, TTSScript(entries=[([-1], 0)]))),
            (ValueError, "padding", lambda: gen.set_session_script(0, TTSScript(entries=[([5], -1)]))),
            (AssertionError, "max_entries", lambda: gen.set_session_script(0, TTSScript(entries=[([5], 0)] * (good.max_entries + 1)))),
            (AssertionError, "max_tokens", lambda: gen.set_session_script(0, TTSScript(entries=[([5] * (good.max_tokens + 1), 0)]))),
            (AssertionError, "max_prefix", lambda: gen.set_session_script(0, TTSScript(entries=[([5], 0)], text_prefix=[5] * 4))),
            (AssertionError, "max_prefix", lambda: gen.set_session_script(0, TTSScript(entries=[([5], 0)], audio_prefix=np.zeros((20, 4), np.int64)))),
            (ValueError, "session", lambda: gen.session_script_status(3)),
        ]
        for exc, match, call in bad:
            with pytest.raises(exc, match=match):
                call()
        assert [gen.session_script_status(b) for b in range(3)] == before, "a refused call changed a status"
        out = np.stack([gen.step(codes_for(gen, 3)).cpu().numpy()[:, :, 0] for _ in range(5)])
    finally:
        gen._stop_streaming()
    ref = tts_gen(device, lib, good)
    try:
        want, _ = run(ref, 3, 8, scripts)
    finally:
        ref._stop_streaming()
    assert np.array_equal(out, want[3:]), "a refused call changed the tokens"


def _capi_status(gen, lib):
    return lib.mmi_lm_set_row_script(gen.lm_model._handle, 0, None, None)
