"""`SessionBatcher` - many live full-duplex sessions on one GPU, host mirror of `mmi_batcher_*`.

The reference's Python server holds one session under a lock (moshi/moshi/server.py:45,57,154-169); its Rust server is the
model for batching: fixed slots, one channel per slot with a PCM FIFO, a model loop that each iteration takes one 80 ms
frame from every channel that has one, resets the rows of channels opened since, runs the batched step under that stream
mask and routes each row's result back (rust/moshi-server/src/batched_asr.rs:188-437, py_module.rs:443-470).  The loop
itself is native (moshi_amd/csrc/batcher.hip); this class only marshals host arrays.

    batcher = SessionBatcher(mimi, lm, slots=32)
    ch = batcher.open()                       # BufferError when every slot is taken
    batcher.push(ch, pcm_float32_24khz)       # any length; frames are cut by the batcher
    batcher.step()                            # one iteration of the model loop (call it from the loop thread)
    frame = batcher.pop(ch)                   # None or (pcm[1920] float32, tokens[1 + dep_q] int64)
    batcher.close(ch)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi
from .errors import UnknownChannel  # noqa: F401  (re-exported: callers catch it from here)
from .lm import LMModel, _apply_logprobs, _apply_nucleus, check_top_p
from .mimi import MimiModel


def _require_duplex_model(cfg, who: str) -> None:
    """Both serving pipelines feed the user's encoded speech in as the n_q - dep_q user codebooks of a duplex model."""
    if cfg.n_q == cfg.dep_q or cfg.demux_second_text_stream:
        raise NotImplementedError(f"{who} serves duplex models (user audio in, n_q > dep_q); a TTS-family model (no user stream "
                                  "or a demuxed text stream) is stepped with LMGen directly")


class SessionBatcher:
    def __init__(self, mimi: MimiModel, lm_model: LMModel, slots: int, use_sampling: bool = True, temp: float = 0.8,
                 temp_text: float = 0.7, top_k: int = 250, top_k_text: int = 25, seed: int = 0,
                 reset_codec_after_first_frame: bool = True, max_buffered_frames: int = 250, cfg_coef: float = 1.0,
                 cfg_is_no_text: bool = False, cfg_is_masked_until=None, condition_tensors=None, top_p: float = 0.0,
                 top_p_text: float = 0.0, session_top_p: bool = False, logprobs: Optional[int] = None):
        assert mimi._lib is lm_model._lib, "both models must live in the same engine library"
        assert not mimi.is_streaming, "the batcher puts the models into streaming mode itself"
        _require_duplex_model(lm_model.config, "SessionBatcher")
        self.mimi, self.lm_model = mimi, lm_model
        self._lib = mimi._lib
        self.frame_size = mimi.frame_size
        self.n_tokens = 1 + lm_model.dep_q
        cfg = _capi.BatcherCfg()
        cfg.slots = int(slots)
        cfg.reset_codec_after_first_frame = 1 if reset_codec_after_first_frame else 0
        cfg.max_buffered_frames = int(max_buffered_frames)
        cfg.sampling.use_sampling = 1 if use_sampling else 0
        cfg.sampling.temp, cfg.sampling.temp_text = temp, temp_text
        cfg.sampling.top_k, cfg.sampling.top_k_text = top_k, top_k_text
        cfg.sampling.seed = seed
        # guidance / conditioning shared by every channel (server.py:53-54 builds ONE set of condition tensors per model type)
        keep = []
        rows = int(slots) * (2 if cfg_coef != 1.0 else 1)
        self._rows = 2 if cfg_coef != 1.0 else 1            # model rows per session
        cfg.guidance.cfg_coef = float(cfg_coef)
        cfg.guidance.cfg_is_no_text = 1 if cfg_is_no_text else 0
        if cfg_is_masked_until is not None and cfg_coef != 1.0:
            mu = (C.c_int64 * int(slots))(*[int(v) for v in cfg_is_masked_until])
            keep.append(mu)
            cfg.guidance.cfg_is_masked_until = C.cast(mu, C.c_void_p)
        if condition_tensors is not None:
            assert lm_model.fuser is not None, "Model has no fuser"
            cs = lm_model.fuser.get_sum(condition_tensors)
            if cs is not None:
                import torch
                assert cs.shape[0] == rows, "one condition row per model row (2 per slot when guided)"
                cs = cs.to(device=lm_model.device, dtype=torch.bfloat16).contiguous().view(rows, lm_model.dim)
                keep.append(cs)
                cfg.guidance.condition_sum = cs.data_ptr()
            cx = lm_model.fuser.get_cross(condition_tensors)
            if cx is not None:
                import torch
                assert cx.shape[0] == rows, "one condition row per model row (2 per slot when guided)"
                cx = cx.to(device=lm_model.device, dtype=torch.bfloat16).contiguous()
                keep.append(cx)
                cfg.guidance.condition_cross = cx.data_ptr()
                cfg.guidance.cross_len = int(cx.shape[1])
        assert mimi.device == lm_model.device, "the codec and the LM of a batcher must live on the same GPU"
        self._handle = C.c_void_p()
        # nucleus sampling: the batcher's own values, and whether channels may bring theirs (SessionSampling.top_p, set_channel_top_p)
        check_top_p(top_p, top_p_text)
        self._nucleus = _apply_nucleus(self._lib, lm_model._handle, float(top_p), float(top_p_text), bool(session_top_p))
        # log-probabilities of every popped frame: None = off, n in 0..8 = on with n alternatives
        self.logprobs = None if logprobs is None else int(logprobs)
        _apply_logprobs(self._lib, lm_model._handle, self.logprobs)
        mimi._sync()
        self._lib.check(self._lib.mmi_batcher_create(mimi._handle, lm_model._handle, C.byref(cfg), C.byref(self._handle)))

    @property
    def nucleus(self) -> bool:
        """Whether the batcher's stream runs the nucleus samplers, i.e. whether channels may bring their own top_p."""
        return self._nucleus

    def close_all(self) -> None:
        """Tear the batcher down (both models leave streaming mode)."""
        if getattr(self, "_handle", None) and self._handle.value:
            self._lib.mmi_batcher_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close_all()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close_all()

    # ---- channels ------------------------------------------------------------------------------------
    def open(self, sampling=None, condition=None, adapter: Optional[int] = None) -> int:
        """Claim a slot.  `sampling`: a `moshi_amd.SessionSampling` - the channel samples with its own settings and its own seeded
        draw stream (the same tokens whichever slot it lands in); None = the batcher's settings.  `condition`: a
        `moshi_amd.SessionCondition` - the channel's own condition tensors (fused like the batcher's; two rows when the batcher
        runs guided; a `cross` source of up to the model's `cross_capacity` positions) and guidance coefficient; None = the
        batcher's own condition for that slot.  `adapter`: the slot of `LMModel(adapters=...)` the channel runs on for its life
        (`close` returns the row to the base model); None = no adapter.  What the engine refuses raises here and claims no slot."""
        ch = C.c_int64(0)
        own_p = sampling is not None and (sampling.top_p > 0 or sampling.top_p_text > 0)
        if sampling is not None:
            check_top_p(sampling.top_p, sampling.top_p_text)
        if own_p and not self._nucleus:
            raise RuntimeError("SessionSampling.top_p > 0 needs a batcher with the nucleus samplers: SessionBatcher(session_top_p=True)")
        if adapter is not None and condition is None:
            sp = C.byref(sampling.to_c()) if sampling is not None else None
            self._lib.check(self._lib.mmi_batcher_open_lora(self._handle, sp, None, int(adapter), C.byref(ch)))
        elif sampling is None and condition is None:
            self._lib.check(self._lib.mmi_batcher_open(self._handle, C.byref(ch)))
        elif condition is None:
            self._lib.check(self._lib.mmi_batcher_open_with(self._handle, C.byref(sampling.to_c()), C.byref(ch)))
        else:
            import torch
            bc = _capi.BatcherCondition()
            bc.cfg_coef = float(condition.cfg_coef)
            keep = []
            if condition.condition_tensors is not None:
                fuser = self.lm_model.fuser
                assert fuser is not None, "Model has no fuser"

                def host(t):            # bf16 bits in host memory: the batcher copies them before the call returns
                    t = t.detach().to(device="cpu", dtype=torch.bfloat16).contiguous()
                    keep.append(t)
                    return t.data_ptr()
                cs = fuser.get_sum(condition.condition_tensors)
                if cs is not None:
                    assert cs.shape[0] == self._rows, "one condition row per model row of a session (2 when guided)"
                    bc.condition_sum = host(cs.reshape(self._rows, self.lm_model.dim))
                cx = fuser.get_cross(condition.condition_tensors)
                if cx is not None:
                    assert cx.shape[0] == self._rows and cx.dim() == 3 and cx.shape[2] == self.lm_model.dim, cx.shape
                    bc.condition_cross = host(cx)
                    bc.cross_len = int(cx.shape[1])
            sp = C.byref(sampling.to_c()) if sampling is not None else None
            if adapter is not None:
                self._lib.check(self._lib.mmi_batcher_open_lora(self._handle, sp, C.byref(bc), int(adapter), C.byref(ch)))
            else:
                self._lib.check(self._lib.mmi_batcher_open_cond(self._handle, sp, C.byref(bc), C.byref(ch)))
        if sampling is not None and self._nucleus:      # the channel's own nucleus values (0 = off for it), before its first step
            try:
                self.set_channel_top_p(int(ch.value), sampling.top_p, sampling.top_p_text)
            except BaseException:
                self._lib.mmi_batcher_close(self._handle, int(ch.value))     # a refused nucleus part leaves no channel open
                raise
        return int(ch.value)

    def fork(self, channel: int, sampling=None) -> int:
        """A new channel that continues from `channel`'s state: both engines' sessions are copied into a free slot on the batcher's
        stream (`LMGen.fork_session`, `MimiModel.fork_session`), between two steps.  The child takes the parent's settings,
        condition, adapter and frame count and starts with empty FIFOs; `sampling`: a `moshi_amd.SessionSampling` of its own - with
        another seed it is another candidate from the same conversation (N-best), without one it repeats the parent under greedy
        or a seeded parent.  Closing the parent leaves the child.  Raises BufferError without a free slot, `UnknownChannel` for an
        unknown parent, RuntimeError for a parent that has not run a step since `open`."""
        own_p = sampling is not None and (sampling.top_p > 0 or sampling.top_p_text > 0)
        if sampling is not None:
            check_top_p(sampling.top_p, sampling.top_p_text)
        if own_p and not self._nucleus:
            raise RuntimeError("SessionSampling.top_p > 0 needs a batcher with the nucleus samplers: SessionBatcher(session_top_p=True)")
        ch = C.c_int64(0)
        sp = C.byref(sampling.to_c()) if sampling is not None else None
        self._lib.check(self._lib.mmi_batcher_fork(self._handle, int(channel), sp, C.byref(ch)))
        if sampling is not None and self._nucleus:
            try:
                self.set_channel_top_p(int(ch.value), sampling.top_p, sampling.top_p_text)
            except BaseException:
                self._lib.mmi_batcher_close(self._handle, int(ch.value))
                raise
        return int(ch.value)

    def set_channel_top_p(self, channel: int, top_p: float, top_p_text: float) -> None:
        """The channel samples with its own nucleus values from the next step on, for its life; `close` returns the row to the
        batcher's values at the following step."""
        self._lib.check(self._lib.mmi_batcher_set_channel_top_p(self._handle, int(channel), float(top_p), float(top_p_text)))

    def close(self, channel: int) -> None:
        self._lib.check(self._lib.mmi_batcher_close(self._handle, int(channel)))

    def push(self, channel: int, pcm) -> None:
        a = np.ascontiguousarray(np.asarray(pcm, dtype=np.float32).reshape(-1))
        self._lib.check(self._lib.mmi_batcher_push_pcm(self._handle, int(channel), a.ctypes.data, a.size))

    def pop(self, channel: int) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        """The channel's next output frame, or None.  A channel that is not (or no longer) open raises `UnknownChannel` - a
        ValueError like every MMI_ERR_INVALID, but one a model loop can tell apart from a real argument error."""
        pcm = np.empty(self.frame_size, dtype=np.float32)
        tok = np.empty(self.n_tokens, dtype=np.int64)
        got = C.c_int32(0)
        self._lib.check(self._lib.mmi_batcher_pop(self._handle, int(channel), pcm.ctypes.data, tok.ctypes.data, C.byref(got)))      # MMI_ERR_NO_CHANNEL -> UnknownChannel
        return (pcm, tok) if got.value else None

    def pop_with_logprobs(self, channel: int):
        """`pop` with the frame's log-probabilities (`SessionBatcher(logprobs=n)`): (pcm, tokens, logp f32 [1 + dep_q], top_ids i64
        [1 + dep_q, n], top_logp f32 [1 + dep_q, n]) or None - `LMGen.frame_logprobs()` of the step that produced the frame."""
        n = self.logprobs or 0
        pcm = np.empty(self.frame_size, dtype=np.float32)
        tok = np.empty(self.n_tokens, dtype=np.int64)
        logp = np.empty(self.n_tokens, dtype=np.float32)
        ids = np.empty((self.n_tokens, n), dtype=np.int32)
        tlp = np.empty((self.n_tokens, n), dtype=np.float32)
        got = C.c_int32(0)
        self._lib.check(self._lib.mmi_batcher_pop_logprobs(self._handle, int(channel), pcm.ctypes.data, tok.ctypes.data, logp.ctypes.data,
                                                           ids.ctypes.data if n else None, tlp.ctypes.data if n else None, C.byref(got)))
        return (pcm, tok, logp, ids.astype(np.int64), tlp) if got.value else None

    # ---- model loop ----------------------------------------------------------------------------------
    def step(self) -> int:
        """One iteration of the model loop; returns the number of rows that had a frame (0 = nothing ran)."""
        n = C.c_int32(0)
        self._lib.check(self._lib.mmi_batcher_step(self._handle, C.byref(n)))
        return int(n.value)

    def stats(self) -> dict:
        s = _capi.BatcherStats()
        self._lib.check(self._lib.mmi_batcher_get_stats(self._handle, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    @property
    def total_slots(self) -> int:      # py_module.rs:643-645
        return self.stats()["total_slots"]

    @property
    def used_slots(self) -> int:       # py_module.rs:647-649
        return self.stats()["used_slots"]
