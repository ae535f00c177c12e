"""`LMModel` / `LMGen` - host-side mirror of the reference's Moshi LM generation API on the HIP engine.

Same constructor arguments, method names, shapes, dtypes, `None`-during-delay behaviour and exception types as
the reference (moshi/moshi/models/lm.py:49-320 `LMModel` attributes, :556-850 `LMGen`), so that callers such as
`server.py:59-72,144` or `run_inference.py:89-90,160-171` can switch.  All arithmetic happens in libmoshi_mi.so.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _capi
from .config import LMConfig


def _lm_cfg_struct(cfg: LMConfig) -> _capi.LMCfg:
    s = _capi.LMCfg()
    s.dim = cfg.dim
    s.num_heads = cfg.num_heads
    s.num_layers = cfg.num_layers
    s.ffn_hidden = cfg.ffn_hidden
    s.context = cfg.context
    s.max_period = cfg.max_period
    s.n_q = cfg.n_q
    s.dep_q = cfg.dep_q
    s.card = cfg.card
    s.text_card = cfg.text_card
    s.text_card_out = cfg.text_card
    s.depformer_dim = cfg.depformer_dim
    s.depformer_num_heads = cfg.depformer_num_heads
    s.depformer_num_layers = cfg.depformer_num_layers
    s.depformer_ffn_hidden = cfg.depformer_ffn_hidden
    assert len(cfg.delays) == cfg.n_q + 1, f"expected {cfg.n_q + 1} delays, got {len(cfg.delays)}."
    for i, d in enumerate(cfg.delays):
        s.delays[i] = d
    s.existing_text_padding_id = cfg.existing_text_padding_id
    s.extra_heads_num_heads = cfg.extra_heads_num_heads
    s.extra_heads_dim = cfg.extra_heads_dim
    if cfg.kv_cache_dtype not in ("bf16", "fp8", "fp4"):
        raise ValueError("kv_cache_dtype must be 'bf16', 'fp8' or 'fp4'")
    if cfg.kv_cache_dtype == "fp4" and (cfg.dim // cfg.num_heads) % 32:
        raise ValueError(f"kv_cache_dtype 'fp4' needs a head dim multiple of 32 (a 16-byte load of the ring is two blocks of 16): "
                         f"dim {cfg.dim} / num_heads {cfg.num_heads} = {cfg.dim // cfg.num_heads}")
    s.kv_cache_dtype = {"bf16": _capi.MMI_BF16, "fp8": _capi.MMI_F8E4M3, "fp4": _capi.MMI_F4E2M1X2}[cfg.kv_cache_dtype]
    s.cross_attention = 1 if cfg.cross_attention else 0
    return s


def _lm_cfg_ext_struct(cfg: LMConfig) -> Optional[_capi.LMCfgExt]:
    """The TTS-family options (mmi_lm_create_ext), or None for a model that has none of them."""
    sched, r = cfg.depformer_weights_per_step_schedule, cfg.depformer_low_rank_embeddings
    if sched is None and not r and not cfg.demux_second_text_stream:
        return None
    x = _capi.LMCfgExt()
    if sched is not None:
        assert len(sched) == cfg.dep_q <= 64, "depformer_weights_per_step_schedule must have dep_q entries"
        for k, v in enumerate(sched):
            x.depformer_schedule[k] = int(v)
        x.depformer_schedule_len = len(sched)
    x.depformer_low_rank = int(r or 0)
    x.demux_second_text_stream = 1 if cfg.demux_second_text_stream else 0
    return x


class ConditionFuser:
    """The part of the reference's `ConditionFuser` that `LMGen` uses (conditioners/base.py:349-421): which named condition
    tensors are summed into the model input (`sum`) and which are concatenated along time into the source every temporal
    layer cross-attends to (`cross`).  `prepend` is not implemented by the reference's generation path either."""

    def __init__(self, fuse2cond: Dict[str, List[str]], cross_attention_pos_emb: bool = False,
                 cross_attention_pos_emb_scale: float = 1.0):
        for method, names in fuse2cond.items():
            if method not in ("sum", "cross", "prepend"):
                raise AssertionError(f"Got invalid fuse method {method}")
            if method == "prepend" and names:
                raise RuntimeError(f"only `sum` and `cross` conditionings are supported for now, got {method}.")   # base.py:380-381
        self.fuse2cond = {"sum": list(fuse2cond.get("sum", [])), "cross": list(fuse2cond.get("cross", [])), "prepend": []}
        self.cross_attention_pos_emb = cross_attention_pos_emb
        self.cross_attention_pos_emb_scale = cross_attention_pos_emb_scale

    def get_sum(self, conditions) -> Optional[torch.Tensor]:
        """conditioners/base.py:410-421: conditions[name] = (tensor [B, 1, dim], mask)."""
        total = None
        for name in self.fuse2cond["sum"]:
            cond = conditions[name][0]
            assert cond.shape[1] == 1, cond.shape
            total = cond if total is None else total + cond
        return total

    def get_cross(self, conditions) -> Optional[torch.Tensor]:
        """conditioners/base.py:392-409: the `cross` conditions concatenated along time, [B, T_c, dim] (+ a sinusoidal
        position embedding when the fuser was built with `cross_attention_pos_emb`)."""
        cross = None
        for name in self.fuse2cond["cross"]:
            cond = conditions[name][0]
            cross = cond if cross is None else torch.cat([cross, cond], dim=1)
        if self.cross_attention_pos_emb and cross is not None:
            positions = torch.arange(cross.shape[1], device=cross.device).view(1, -1, 1)
            half = cross.shape[-1] // 2                     # modules/transformer.py:139-164 create_sin_embedding
            adim = torch.arange(half, device=cross.device, dtype=torch.float32).view(1, 1, -1)
            phase = positions.to(torch.float32) / (torch.full([], 10000.0, device=cross.device) ** (adim / (half - 1)))
            pos_emb = torch.cat([torch.cos(phase), torch.sin(phase)], dim=-1).to(cross.dtype)
            cross = cross + self.cross_attention_pos_emb_scale * pos_emb
        return cross


class LMModel:
    """Weights + architecture of the Moshi LM on the engine (reference: lm.py:49-320).

    Args:
        state_dict: bf16 tensors named as in the reference checkpoints.
        config: architecture hyper-parameters (defaults = Moshi-7B, loaders.py:90-119).
        device: a ROCm `cuda` device for the product library.
        max_batch: largest number of concurrent sessions `LMGen.streaming` will be asked for (at most 64).
        max_rows: instead of `max_batch`, a handle of up to 128 MODEL rows (mmi_lm_create_rows; bf16 linears): sessions, or two
            rows per guided session.  `lm.max_batch` then reports it.  Not together with `max_batch > 64`.
        quantize: True converts the linears to row-wise int8 (`weight` + `weight_scb`), like the reference's `quantize=True`;
            "fp8" converts them to e4m3fn (`weight` + `weight_scale`) for the fp8 MFMA path (BASELINE configs[4]);
            "mxfp4" converts them to OCP MXFP4 (`weight` uint8 code pairs + `weight_scale_e8m0`; weight-only, widened to bf16 in
            the GEMM - exactly the bf16 engine on `dequantize_lm_state_dict_mxfp4`); in_features must be multiples of 32;
            a state dict that already carries int8 / fp8 / MXFP4 weights is used as is.
        adapters: (max_adapters, max_rank) - room for up to 8 LoRA adapters of rank <= 32 / 64 / 96 / 128 NEXT TO this base model,
            chosen per session (`load_adapter`, `LMGen.set_session_adapter`; modules/lora.py, unmerged).  bf16 linears, at most 64
            model rows, no cross-attention layers, no extra heads.  None: a plain handle.
        prefill_rows: the row budget (1..128) of one pass of `LMGen.prefill` (mmi_lm_enable_prefill): known frames
            enter a session `prefill_rows` rows at a time, one pass over the temporal weights each.  bf16 linears, no
            cross-attention layers, no adapters, no TTS machine; above 32 the handle must be built for more than 16 rows.
            None: off - the handle allocates and launches what it always did.
        score: True (with `prefill_rows`) enables `LMGen.score` (mmi_lm_enable_score): teacher-forced scoring of
            known frames on the prefill pass, with scratch of its own beside the prefill scratch.  Plain (not low-rank, not demuxed)
            depformer embeddings.  False: the handle allocates and launches what a prefill handle does.
    """

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: Optional[LMConfig] = None,
                 device: torch.device | str = "cuda", max_batch: int = 32, lib: Optional[_capi.Lib] = None,
                 quantize: bool | str = False, fuser: Optional[ConditionFuser] = None, kv_cache: Optional[str] = None,
                 cross_capacity: Optional[int] = None, max_rows: Optional[int] = None,
                 adapters: Optional[Tuple[int, int]] = None, prefill_rows: Optional[int] = None, score: bool = False):
        if max_rows is not None:
            if max_batch > 64:
                raise ValueError("max_rows and max_batch > 64 are mutually exclusive: max_rows alone sizes the handle")
            if int(max_rows) < 1:
                raise ValueError("max_rows must be >= 1")
            max_batch = int(max_rows)
        self.config = config or LMConfig()
        if kv_cache is not None:         # "fp8": e4m3 KV ring (half the attention stream); "fp4": E2M1 codes under block scales
                                         # (0.5625 bytes per element); default: the config's (bf16)
            from dataclasses import replace
            self.config = replace(self.config, kv_cache_dtype=kv_cache)
        self.fuser = fuser
        self.device = torch.device(device)
        if lib is None:
            if self.device.type != "cuda":
                raise RuntimeError("moshi_amd.LMModel runs on an MI355X (device='cuda'); there is no CPU path")
            lib = _capi.load()
        self._lib = lib
        self._handle = C.c_void_p()
        from .weights import (is_mxfp4_state_dict, normalize_lm_state_dict, quantize_lm_state_dict, quantize_lm_state_dict_fp8,
                              quantize_lm_state_dict_mxfp4)
        state_dict = normalize_lm_state_dict(state_dict, self.config)     # fused multi-step projections of released checkpoints
        if quantize == "fp8":
            state_dict = quantize_lm_state_dict_fp8(state_dict)
        elif quantize == "mxfp4":
            state_dict = quantize_lm_state_dict_mxfp4(state_dict)
        elif quantize:                                                    # the reference's `quantize=True` (lm.py:242-243)
            state_dict = quantize_lm_state_dict(state_dict)
        self.quantized = any(v.dtype in (torch.int8, torch.float8_e4m3fn) for v in state_dict.values()) or is_mxfp4_state_dict(state_dict)
        if self.quantized and getattr(config, "cross_attention", False):
            # the engine runs one weight format per model (activation buffers are laid out for it) and keeps cross-attention
            # linears bf16: fail here, with the reason, instead of inside mmi_lm_create
            raise NotImplementedError("quantised linears (int8 / fp8) are not supported for models with cross-attention layers; "
                                      "load the bf16 checkpoint (quantize=False)")
        if self.quantized and (self.config.depformer_low_rank_embeddings or self.config.demux_second_text_stream):
            # the reference would quantise the `low_rank` / `out1` / `out2` linears as well (utils/quantize.py): not built
            raise NotImplementedError("quantised linears (int8 / fp8) are not supported with low-rank or demuxed embeddings; "
                                      "load the bf16 checkpoint (quantize=False)")

        def place(k, v):     # quantised weights and their fp32 scales keep their dtype (utils/quantize.py:29-34); the rest is bf16
            if v.dtype in (torch.int8, torch.float8_e4m3fn, torch.uint8):
                return v.detach().to(self.device)
            scale = k.endswith("_scb") or k.endswith(".weight_scale") or k.endswith(".input_scale")
            return v.detach().to(device=self.device, dtype=torch.float32 if scale else torch.bfloat16)
        sd = {k: place(k, v) for k, v in state_dict.items()}
        descs, keep = _capi.tensor_descs(sd)
        cfg = _lm_cfg_struct(self.config)
        ext = _lm_cfg_ext_struct(self.config)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        with _capi.device_scope(self.device):             # the handle binds to the device current at create
            if max_rows is not None:
                lib.check(lib.mmi_lm_create_rows(C.byref(cfg), C.byref(ext) if ext is not None else None, descs, len(sd), max_batch,
                                                 C.byref(self._handle)))
            elif ext is None:
                lib.check(lib.mmi_lm_create(C.byref(cfg), descs, len(sd), max_batch, C.byref(self._handle)))
            else:
                lib.check(lib.mmi_lm_create_ext(C.byref(cfg), C.byref(ext), descs, len(sd), max_batch, C.byref(self._handle)))
        del keep, sd
        if self.config.existing_text_end_padding_id != 0:     # the one id of the text history's skip list that the cfg struct does not carry
            lib.check(lib.mmi_lm_set_text_end_padding_id(self._handle, int(self.config.existing_text_end_padding_id)))
        self.max_batch = max_batch
        self.training = False
        if cross_capacity is not None:
            self.set_cross_capacity(cross_capacity)
        self.adapters = None
        if adapters is not None:
            max_adapters, max_rank = adapters
            lib.check(lib.mmi_lm_enable_adapters(self._handle, int(max_adapters), int(max_rank)))
            self.adapters = (int(max_adapters), int(max_rank))
        self.prefill_rows = None
        if prefill_rows is not None:
            lib.check(lib.mmi_lm_enable_prefill(self._handle, int(prefill_rows)))
            self.prefill_rows = int(prefill_rows)
        self.score = False
        if score:
            lib.check(lib.mmi_lm_enable_score(self._handle, 1))
            self.score = True

    def __del__(self):
        try:
            if getattr(self, "_handle", None) and self._handle.value:
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
                self._lib.mmi_lm_destroy(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass

    def set_cross_capacity(self, positions: Optional[int]) -> None:
        """Positions a session's cross-attention source may hold in the streams started from now on (`LMModel(cross_capacity=)`):
        room for `LMGen.set_session_condition` / `SessionBatcher.open(condition=)` to bring a longer source than the one the
        stream starts with.  None or 0 = the length of the start's source.  Not while streaming."""
        self._lib.check(self._lib.mmi_lm_set_cross_capacity(self._handle, int(positions or 0)))

    # ---- LoRA adapters next to the base model (mmi_lm_enable_adapters) ---------------------------------
    def load_adapter(self, slot: int, lora_state_dict: Dict[str, torch.Tensor], scaling: float = 2.0) -> None:
        """Adapter `slot` = `<linear>.lora_A.weight` [r, in] / `<linear>.lora_B.weight` [out, r] of `lora_state_dict` (the keys of a
        reference LoRA checkpoint; fused multi-step projections are split like the base weights'), run unmerged as
        `frozen_W(x) + lora_B(lora_A(x)) * scaling` (modules/lora.py:116-118) for the sessions that select it.  Allowed while
        streaming; refused while a live session runs on the slot.  Unknown keys, shapes that do not fit, a rank above the
        handle's or values that are not finite raise ValueError and leave the slot as it was."""
        from .weights import normalize_lm_state_dict
        sd = normalize_lm_state_dict(dict(lora_state_dict), self.config)
        sd = {k: v.detach().to(device=self.device, dtype=torch.bfloat16).contiguous() for k, v in sd.items()}
        descs, keep = _capi.tensor_descs(sd)
        self._lib.check(self._lib.mmi_lm_load_adapter(self._handle, int(slot), float(scaling), descs, len(sd), _capi.stream_ptr(self.device)))
        if self.device.type == "cuda":          # the packing launches read the tensors: keep them until it has run
            torch.cuda.current_stream(self.device).synchronize()
        del keep, sd

    def unload_adapter(self, slot: int) -> None:
        """Zeroes adapter `slot` (refused while a live session runs on it)."""
        self._lib.check(self._lib.mmi_lm_unload_adapter(self._handle, int(slot), _capi.stream_ptr(self.device)))

    def debug_linear_lora(self, weight_name: str, x: torch.Tensor, row_slots: Sequence[int], path: str = "plain") -> dict:
        """`debug_linear` on an adapter handle (tests; `mmi_lm_debug_linear_lora`): the shrink launch plus the GEMM of that linear as
        the step runs them, row b on adapter slot `row_slots[b]` (-1 = none).  Paths "plain" and "splitk"."""
        x = x.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, K = x.shape
        assert K == self._linear_in_features(weight_name), f"{weight_name} takes rows of {self._linear_in_features(weight_name)} features, got {K}"
        assert len(row_slots) == rows, "one adapter slot per row"
        out = torch.empty(rows, self._linear_out_features(weight_name), dtype=torch.bfloat16, device=self.device)
        slots = (C.c_int32 * rows)(*[int(v) for v in row_slots])
        self._lib.check(self._lib.mmi_lm_debug_linear_lora(self._handle, weight_name.encode(), None, self.DEBUG_PATHS[path], x.data_ptr(), rows,
                                                           out.data_ptr(), None, None, None, slots, _capi.stream_ptr(self.device)))
        return {"out": out}

    def enable_hidden_taps(self, on: bool = True) -> None:
        """Parity tap (tests): every step of the NEXT `LMGen.streaming()` also keeps the residual stream after the first and
        the last temporal layer (`LMGen.hidden_taps()`)."""
        self._lib.check(self._lib.mmi_lm_set_hidden_taps(self._handle, 1 if on else 0))

    DEBUG_PATHS = {"plain": 0, "splitk": 1, "fused": 2, "norm": 3, "norm_fused": 4}

    def debug_kv4_quantize(self, x: torch.Tensor):
        """Test aid (`mmi_lm_debug_kv4_quantize`): the device quantiser of the 4-bit KV ring on bf16 rows [n, 16 * m] ->
        (codes uint8 [n, 8 * m], scale bytes uint8 [n, m])."""
        x = x.to(device=self.device, dtype=torch.bfloat16).contiguous()
        assert x.dim() == 2 and x.shape[1] % 16 == 0, "rows of whole blocks of 16"
        n, m = x.shape[0], x.shape[1] // 16
        codes = torch.empty(n, 8 * m, dtype=torch.uint8, device=self.device)
        scales = torch.empty(n, m, dtype=torch.uint8, device=self.device)
        self._lib.check(self._lib.mmi_lm_debug_kv4_quantize(self._handle, x.data_ptr(), n, m, codes.data_ptr(), scales.data_ptr(),
                                                            _capi.stream_ptr(self.device)))
        return codes, scales

    ATTN_RING_FORMS = {"bf16": _capi.MMI_BF16, "fp8": _capi.MMI_F8E4M3, "fp4": _capi.MMI_F4E2M1X2}

    def debug_attn(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, offsets: torch.Tensor, cap: int, context: Optional[int] = None,
                   ring: str = "bf16", kernel: str = "wave", ns: int = 1, merge: str = "launch", solo_rows: int = -1) -> torch.Tensor:
        """Parity tap (tests; `mmi_lm_debug_attn`): the temporal decode attention alone, through the step's own dispatch, on
        caller-supplied operands.  `q` bf16 [rows, H, Dh] (already roped); `k`, `v` uint8, the ring bytes in the layout of
        `debug_kv_ring` for `cap` slots (bf16 [rows, H, cap, Dh]; "fp8" the same in bytes; "fp4" the codes plane, then the scale
        plane); `offsets` int64 [rows].  `kernel` "wave" / "split", `ns` workgroups per (row, head), `merge` "launch"
        (`k_lm_attn_combine`) or "kernel" (the last-arriving workgroup; rings of at most `solo_rows` rows are walked by workgroup 0
        alone).  Returns bf16 [rows, H * Dh].  Independent of the handle's model and of any running stream."""
        q = q.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, H, Dh = q.shape
        k, v = (t.to(device=self.device).contiguous().view(torch.uint8).reshape(-1) for t in (k, v))
        per_elem = {"bf16": 32, "fp8": 16, "fp4": 9}[ring]                 # sixteenths of a byte
        want = rows * H * int(cap) * Dh * per_elem // 16
        assert k.numel() == want and v.numel() == want, f"a {ring} ring of {rows} x {H} x {cap} x {Dh} is {want} bytes, got {k.numel()} / {v.numel()}"
        offsets = offsets.to(device=self.device, dtype=torch.int64).contiguous()
        assert offsets.shape == (rows,), "one offset per row"
        out = torch.empty(rows, H * Dh, dtype=torch.bfloat16, device=self.device)
        self._lib.check(self._lib.mmi_lm_debug_attn(
            self._handle, q.data_ptr(), k.data_ptr(), v.data_ptr(), offsets.data_ptr(), rows, H, Dh, int(cap),
            int(cap if context is None else context), self.ATTN_RING_FORMS[ring], {"wave": 0, "split": 1}[kernel], int(ns),
            {"launch": 0, "kernel": 1}[merge], int(solo_rows), out.data_ptr(), _capi.stream_ptr(self.device)))
        return out

    DEP_ATTN_KERNELS = {"auto": 0, "attn8": 1, "rows16": 2, "rows32": 3, "fused": 4}
    _DEP_ATTN_NAMES = {v: k for k, v in DEP_ATTN_KERNELS.items()}

    def debug_dep_attn(self, qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, H: int, k: int, kernel: str = "auto"):
        """Parity tap (tests; `mmi_lm_debug_dep_attn`): micro-step `k` of the depth transformer's attention alone, through the launch
        function of the step and of the scoring pass.  `qkv` bf16 [rows, 3 * H * Dh]; `kc`, `vc` bf16 [rows, H, steps, Dh], device
        tensors that are read and WRITTEN in place (row k).  `kernel` "auto" (the step's choice) / "attn8" / "rows16" / "rows32".
        Returns (bf16 [rows, H * Dh], the name of the kernel that ran)."""
        qkv = qkv.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, steps, Dh = kc.shape[0], kc.shape[2], kc.shape[3]
        for c in (kc, vc):
            assert c.dtype == torch.bfloat16 and c.is_contiguous() and c.device == qkv.device and c.shape == (rows, H, steps, Dh), \
                "the caches are contiguous bf16 [rows, H, steps, Dh] on the handle's device (they are written in place)"
        assert qkv.shape == (rows, 3 * H * Dh), "qkv is [rows, 3 * H * Dh]"
        out = torch.empty(rows, H * Dh, dtype=torch.bfloat16, device=self.device)
        ran = C.c_int32(-1)
        self._lib.check(self._lib.mmi_lm_debug_dep_attn(self._handle, qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), rows, int(H), Dh, steps,
                                                        int(k), self.DEP_ATTN_KERNELS[kernel], out.data_ptr(), C.byref(ran),
                                                        _capi.stream_ptr(self.device)))
        return out, self._DEP_ATTN_NAMES[ran.value]

    def debug_dep_attn_out_proj(self, layer: int, k: int, qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, x: torch.Tensor,
                                fused: bool = True):
        """Parity tap (tests; `mmi_lm_debug_dep_attn_out_proj`): x + out_proj(attention) of one row with the out_proj weight of depth
        layer `layer`, micro-step `k` >= 1 of this model - `fused`: the attention inside the GEMM (k_dep_attn_out_proj), else the two
        launches it replaces.  `qkv` bf16 [3 * dd], `kc` / `vc` bf16 [H, dep_q, Dh] (written in place), `x` bf16 [dd].
        Returns (bf16 [dd], the attention output bf16 [dd] of the two-launch form or None, the name of the kernel that ran)."""
        qkv, x = (t.to(device=self.device, dtype=torch.bfloat16).contiguous().reshape(-1) for t in (qkv, x))
        dd = x.numel()
        assert qkv.numel() == 3 * dd, "qkv is [3 * depformer_dim]"
        for c in (kc, vc):
            assert c.dtype == torch.bfloat16 and c.is_contiguous() and c.device == qkv.device and c.numel() == dd * self.config.dep_q, \
                "the caches are contiguous bf16 [H, dep_q, Dh] on the handle's device (they are written in place)"
        out = torch.empty(dd, dtype=torch.bfloat16, device=self.device)
        att = None if fused else torch.empty(dd, dtype=torch.bfloat16, device=self.device)
        ran = C.c_int32(-1)
        self._lib.check(self._lib.mmi_lm_debug_dep_attn_out_proj(
            self._handle, int(layer), int(k), 1 if fused else 0, qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), x.data_ptr(), out.data_ptr(),
            None if fused else att.data_ptr(), C.byref(ran), _capi.stream_ptr(self.device)))
        return out, att, self._DEP_ATTN_NAMES[ran.value]

    def debug_cross_attn(self, q: torch.Tensor, kv: torch.Tensor, length: torch.Tensor) -> torch.Tensor:
        """Parity tap (tests; `mmi_lm_debug_cross_attn`): the cross attention alone, through the step's launch function.  `q` bf16
        [rows, H, Dh]; `kv` bf16 [rows, cap, 2 * H * Dh] (keys, then values); `length` int32 [rows], each in [1, cap].
        Returns bf16 [rows, H * Dh]."""
        q = q.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, H, Dh = q.shape
        kv = kv.to(device=self.device, dtype=torch.bfloat16).contiguous()
        assert kv.dim() == 3 and kv.shape[0] == rows and kv.shape[2] == 2 * H * Dh, "kv is [rows, cap, 2 * H * Dh]"
        length = length.to(device=self.device, dtype=torch.int32).contiguous()
        assert length.shape == (rows,), "one length per row"
        out = torch.empty(rows, H * Dh, dtype=torch.bfloat16, device=self.device)
        self._lib.check(self._lib.mmi_lm_debug_cross_attn(self._handle, q.data_ptr(), kv.data_ptr(), length.data_ptr(), rows, H, Dh,
                                                          int(kv.shape[1]), out.data_ptr(), _capi.stream_ptr(self.device)))
        return out

    def debug_prefill_attn(self, q: torch.Tensor, row_ring: torch.Tensor, row_pos: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                           k_staged: torch.Tensor, v_staged: torch.Tensor, cap: int, context: Optional[int] = None, ring: str = "bf16",
                           n_blocks: int = 1, rings: int = 1) -> torch.Tensor:
        """Parity tap (tests; `mmi_lm_debug_prefill_attn`): the prefill attention alone, through the launch function of a prefill pass.
        `q` bf16 [rows, H, Dh] (already roped); `row_ring` int32 [rows] / `row_pos` int64 [rows]: the row table of a pass, `n_blocks`
        equal blocks, each naming one of `rings` rings and consecutive positions; `k`, `v` uint8: the rings in the layout of
        `debug_kv_ring` for `cap` slots; `k_staged`, `v_staged` uint8: the block in ring format ([rows, H, row bytes], then a 4-bit
        ring's scale bytes [rows, H, Dh / 16]).  Returns bf16 [rows, H * Dh]."""
        q = q.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, H, Dh = q.shape
        k, v, ks, vs = (t.to(device=self.device).contiguous().view(torch.uint8).reshape(-1) for t in (k, v, k_staged, v_staged))
        per_elem = {"bf16": 32, "fp8": 16, "fp4": 9}[ring]                 # sixteenths of a byte
        want = int(rings) * H * int(cap) * Dh * per_elem // 16
        assert k.numel() == want and v.numel() == want, f"{rings} {ring} rings of {H} x {cap} x {Dh} are {want} bytes, got {k.numel()} / {v.numel()}"
        want = rows * H * Dh * per_elem // 16
        assert ks.numel() == want and vs.numel() == want, f"a staged {ring} block of {rows} x {H} x {Dh} is {want} bytes, got {ks.numel()} / {vs.numel()}"
        row_ring = row_ring.to(device=self.device, dtype=torch.int32).contiguous()
        row_pos = row_pos.to(device=self.device, dtype=torch.int64).contiguous()
        assert row_ring.shape == (rows,) and row_pos.shape == (rows,), "one ring and one position per row"
        out = torch.empty(rows, H * Dh, dtype=torch.bfloat16, device=self.device)
        self._lib.check(self._lib.mmi_lm_debug_prefill_attn(
            self._handle, q.data_ptr(), row_ring.data_ptr(), row_pos.data_ptr(), k.data_ptr(), v.data_ptr(), ks.data_ptr(), vs.data_ptr(),
            rows, int(n_blocks), int(rings), H, Dh, int(cap), int(cap if context is None else context), self.ATTN_RING_FORMS[ring],
            out.data_ptr(), _capi.stream_ptr(self.device)))
        return out

    def debug_score_rows(self, logits: torch.Tensor, targets: torch.Tensor, want_f32: bool = True):
        """Parity tap (tests; `mmi_lm_debug_score_rows`): the output kernel of `LMGen.score` alone, through the launch function of a
        scoring pass.  `logits` bf16 [rows, N] (N a multiple of 8, at most 32768), `targets` int32 [rows].  Returns (logp f32 [rows],
        argmax int32 [rows], the rows widened to f32 [rows, N] or None)."""
        logits = logits.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, N = logits.shape
        targets = targets.to(device=self.device, dtype=torch.int32).contiguous()
        assert targets.shape == (rows,), "one given token per row"
        logp = torch.empty(rows, dtype=torch.float32, device=self.device)
        argmax = torch.empty(rows, dtype=torch.int32, device=self.device)
        wide = torch.empty(rows, N, dtype=torch.float32, device=self.device) if want_f32 else None
        self._lib.check(self._lib.mmi_lm_debug_score_rows(self._handle, logits.data_ptr(), targets.data_ptr(), rows, N, logp.data_ptr(),
                                                          argmax.data_ptr(), wide.data_ptr() if want_f32 else None,
                                                          _capi.stream_ptr(self.device)))
        return logp, argmax, wide

    def debug_step_logprob(self, logits: torch.Tensor, targets: torch.Tensor, top_n: int = 0) -> "LogProbs":
        """Parity tap (tests; `mmi_lm_debug_step_logprob`): the log-probability op of the step alone, through its launch function.
        `logits` bf16 [rows, N] (N a multiple of 8, at most 32768), `targets` int32 [rows].  Returns LogProbs with logp f32 [rows],
        top_ids i64 / top_logp f32 [rows, top_n]."""
        logits = logits.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, N = logits.shape
        targets = targets.to(device=self.device, dtype=torch.int32).contiguous()
        assert targets.shape == (rows,), "one token per row"
        logp = torch.empty(rows, dtype=torch.float32, device=self.device)
        ids = torch.empty(rows, int(top_n), dtype=torch.int32, device=self.device)
        tlp = torch.empty(rows, int(top_n), dtype=torch.float32, device=self.device)
        some = 0 < int(top_n) <= 8
        self._lib.check(self._lib.mmi_lm_debug_step_logprob(self._handle, logits.data_ptr(), targets.data_ptr(), rows, N, int(top_n),
                                                            logp.data_ptr(), ids.data_ptr() if some else None,
                                                            tlp.data_ptr() if some else None, _capi.stream_ptr(self.device)))
        return LogProbs(logp, ids.to(torch.int64), tlp)

    def debug_linear(self, weight_name: str, x: torch.Tensor, path: str = "plain", alpha_name: Optional[str] = None,
                     want_codes: bool = False) -> dict:
        """Parity tap (tests; `mmi_lm_debug_linear`): ONE linear of the model - the module stored under `weight_name`, i.e.
        `F.linear` / `QLinear.forward` (utils/quantize.py:24-40) - on the bf16 rows `x` [rows, in_features], through the kernels
        the step uses for it.  Returns {"out": bf16 [rows, out_features] (a gated linear_in: silu(gate) * value), and on request
        "codes" int8 [rows, in_features] / "absmax" fp32 [rows] (the row-wise quantisation the int8 x int8 GEMM consumed),
        "norm": the normalised rows (path "norm")}."""
        lib = self._lib
        x = x.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows, K = x.shape
        # the C entry sizes its operand from the packed weight: rows of another width would be read and written out of bounds
        assert K == self._linear_in_features(weight_name), f"{weight_name} takes rows of {self._linear_in_features(weight_name)} features, got {K}"
        w = weight_name.encode()
        # out_features from the config-independent side: ask for a generous buffer, the engine writes [rows][N]
        n_out = self._linear_out_features(weight_name)
        out = torch.empty(rows, n_out, dtype=torch.bfloat16, device=self.device)
        codes = torch.empty(rows, K, dtype=torch.int8, device=self.device) if want_codes else None
        absmax = torch.empty(rows, dtype=torch.float32, device=self.device) if want_codes else None
        norm = torch.empty(rows, K, dtype=torch.bfloat16, device=self.device) if path == "norm" else None
        ptr = lambda t: None if t is None else t.data_ptr()
        lib.check(lib.mmi_lm_debug_linear(self._handle, w, alpha_name.encode() if alpha_name else None, self.DEBUG_PATHS[path],
                                          x.data_ptr(), rows, out.data_ptr(), ptr(codes), ptr(absmax), ptr(norm),
                                          _capi.stream_ptr(self.device)))
        res = {"out": out}
        if want_codes:
            res.update(codes=codes, absmax=absmax)
        if norm is not None:
            res["norm"] = norm
        return res

    def _linear_in_features(self, weight_name: str) -> int:
        c = self.config
        dep = weight_name.startswith("depformer.") or weight_name.startswith("linears.")
        if "linear_out" in weight_name:
            return c.depformer_ffn_hidden if dep else c.ffn_hidden
        return c.depformer_dim if dep else c.dim          # (depformer_in.* and text_linear read the temporal transformer's output)

    def _linear_out_features(self, weight_name: str) -> int:
        c = self.config
        dd = c.depformer_dim
        dep = weight_name.startswith("depformer.")
        d = dd if dep else c.dim
        if ".self_attn.in_projs." in weight_name:
            return 3 * d
        if ".self_attn.out_projs." in weight_name:
            return d
        if "linear_in" in weight_name:           # gated: the engine returns the hidden tensor
            return c.depformer_ffn_hidden if dep else c.ffn_hidden
        if "linear_out" in weight_name:
            return d
        if weight_name.startswith("text_linear"):
            return c.text_card
        if weight_name.startswith("depformer_in."):
            return dd
        if weight_name.startswith("linears."):
            return c.card
        raise KeyError(weight_name)

    # attributes callers read
    @property
    def dep_q(self) -> int:
        return self.config.dep_q

    @property
    def n_q(self) -> int:
        return self.config.n_q

    @property
    def card(self) -> int:
        return self.config.card

    @property
    def text_card(self) -> int:
        return self.config.text_card

    @property
    def delays(self) -> List[int]:
        return list(self.config.delays)

    @property
    def dim(self) -> int:
        return self.config.dim

    @property
    def dtype(self) -> torch.dtype:
        return torch.bfloat16

    @property
    def num_codebooks(self) -> int:
        return self.config.n_q + 1

    @property
    def num_audio_codebooks(self) -> int:
        return self.config.n_q

    @property
    def audio_offset(self) -> int:
        return 1

    @property
    def initial_token_id(self) -> int:
        return self.config.card

    @property
    def text_initial_token_id(self) -> int:
        return self.config.text_card

    @property
    def text_padding_token_id(self) -> int:
        return self.config.existing_text_padding_id

    @property
    def end_of_text_padding_id(self) -> int:
        # lm.py:260-263: the constructor's `existing_text_end_padding_id` (default 0), carried by LMConfig / loaders
        return self.config.existing_text_end_padding_id

    @property
    def existing_text_padding_id(self) -> int:
        return self.config.existing_text_padding_id

    # lm.py:176-183 builds a ConditionProvider from the checkpoint's `conditioners`; turning attributes (a speaker wav, a text
    # description) into tensors is not on the frame step and is out of scope here.  Callers that branch on
    # `lm.condition_provider is not None` (run_inference.py:38, tts.py:449-460) see None and pass `condition_tensors` to LMGen.
    condition_provider = None

    def set_streaming_detached(self, streaming_detached: bool) -> None:
        """streaming.py:78-86.  The reference detaches a module so that a parent's `.streaming()` does not reach it; an engine
        handle has no parent module and is only ever put into streaming mode by a direct call, i.e. it is always detached."""
        self._streaming_detached = bool(streaming_detached)

    @property
    def zero_token_id(self) -> int:
        return -1

    @property
    def ungenerated_token_id(self) -> int:
        return -2


@dataclass
class SessionSampling:
    """One session's own sampling settings (the reference's Rust server reads them from each connection's query string,
    rust/moshi-backend/src/stream_both.rs:95-105).  `seed` keys the session's own draw stream: its tokens do not depend on the
    slot it runs in.  `pad_mult` biases the text padding token (0 = off), `repetition_penalty` (1 = off) applies to the distinct
    tokens among the session's last `repetition_context` (<= 64, 0 = off) text tokens; both act on the text logits only."""
    use_sampling: bool = True
    temp: float = 0.8
    temp_text: float = 0.7
    top_k: int = 250
    top_k_text: int = 25
    seed: int = 0
    pad_mult: float = 0.0
    repetition_penalty: float = 1.0
    repetition_context: int = 0
    # The session's own nucleus (0 = off; > 0 overrides its top_k): applied through mmi_lm_set_row_top_p, not part of to_c().  Like
    # every field here they are the SESSION's values: a SessionSampling with the defaults gives the session top_p = 0 even where the
    # stream's own top_p is positive (on a nucleus stream; the C calls keep the two tables apart - use set_session_top_p for the
    # nucleus alone)
    top_p: float = 0.0
    top_p_text: float = 0.0

    def to_c(self) -> "_capi.RowSampling":
        r = _capi.RowSampling()
        r.use_sampling = 1 if self.use_sampling else 0
        r.temp, r.temp_text = float(self.temp), float(self.temp_text)
        r.top_k, r.top_k_text = int(self.top_k), int(self.top_k_text)
        r.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        r.pad_mult, r.repetition_penalty = float(self.pad_mult), float(self.repetition_penalty)
        r.repetition_context = int(self.repetition_context)
        return r

    def validate(self) -> None:
        """The engine's own rules (mmi_row_sampling_check), restated so that a caller without a handle - the server, while it
        parses a connection's query string - can refuse early with the same exception types."""
        import math
        if self.top_k > 256 or self.top_k_text > 256:
            raise NotImplementedError("top_k > 256")
        if self.top_k < 0 or self.top_k_text < 0:
            raise ValueError("top_k must be >= 0 (0 = no top-k)")
        if not 0 <= self.repetition_context <= 64:
            raise ValueError("repetition_context must be in [0, 64]")
        if not all(math.isfinite(float(v)) for v in (self.temp, self.temp_text, self.pad_mult, self.repetition_penalty)):
            raise ValueError("per-session sampling settings must be finite")
        if not self.repetition_penalty > 0:
            raise ValueError("repetition_penalty must be > 0 (1 = off)")
        check_top_p(self.top_p, self.top_p_text)


def check_top_p(top_p: float, top_p_text: float) -> None:
    """The domain of the two nucleus values (mmi_lm_set_top_p): [0, 1], 0 = off."""
    import math
    for v in (top_p, top_p_text):
        if not (math.isfinite(float(v)) and 0.0 <= float(v) <= 1.0):
            raise ValueError("top_p and top_p_text must lie in [0, 1] (0 = off)")


@dataclass
class SessionCondition:
    """One session's own condition and guidance strength (the reference's Rust TTS server takes the voice source and `cfg_alpha`
    from each request, rust/moshi-server/src/tts.rs:342-357).  `condition_tensors`: as for `LMGen`, fused through the model's
    fuser - one row, or two (conditioned, then unconditioned) on a stream under guidance; None keeps what the session has.  A
    `cross` source may have any length up to the model's `cross_capacity`.  `cfg_coef` 1 = the session's sampling sites keep the
    conditioned logits untouched; another value needs a stream that was started with guidance."""
    cfg_coef: float = 1.0
    condition_tensors: Optional[dict] = None


@dataclass
class LogProbs:
    """What `LMGen.last_logprobs` / `LMGen.frame_logprobs` return; site 0 is the text head, sites 1 .. dep_q the
    audio heads, n the alternatives the stream records."""
    logp: torch.Tensor                       # f32 [B, 1 + dep_q]: ln softmax(logits)[stored token]; -inf outside the head's range; NaN = nothing recorded
    top_ids: torch.Tensor                    # i64 [B, 1 + dep_q, n]: the first n in the order (logit descending, index ascending); -1 = nothing recorded
    top_logp: torch.Tensor                   # f32 [B, 1 + dep_q, n]


def _apply_logprobs(lib, handle, logprobs: Optional[int]) -> None:
    """`logprobs=None | 0..8` onto the handle, before a stream starts (the option belongs to the handle, like the TTS machine)."""
    if logprobs is None and not hasattr(lib.cdll, "mmi_lm_enable_logprobs"):
        return                                            # an older build of the engine has nothing to switch off
    lib.check(lib.mmi_lm_enable_logprobs(handle, 0 if logprobs is None else 1, 0 if logprobs is None else int(logprobs)))


@dataclass
class ScoreOutput:
    """What `LMGen.score` returns for n sessions and T frames; site 0 is the text head, sites 1 .. dep_q the audio heads."""
    logp: torch.Tensor                       # f32 [n, 1 + dep_q, T]: ln softmax(logits)[given token]; -inf outside the head's range
    argmax: torch.Tensor                     # i64 [n, 1 + dep_q, T]: the lowest index among the largest logits
    text_logits: Optional[torch.Tensor]      # f32 [n, T, text_card] with return_logits, else None
    audio_logits: Optional[torch.Tensor]     # f32 [n, T, dep_q, card] with return_logits (None when dep_q == 0), else None


@dataclass
class TTSMachine:
    """The settings of the reference's `StateMachine` and of `TTSModel.generate`'s hooks (models/tts.py:37-57, 146-149, 553-570),
    run on the device per session (mmi_lm_enable_tts_machine).  `text_card` is `TokenIds.card`, the mux base of a demuxed text
    stream (the model's text_card + 1).  The capacities size every session's script: entries, tokens over all entries, prefix
    columns."""
    text_card: int
    new_word: int = 0
    pad: int = 3
    zero: int = -1
    second_stream_ahead: int = 0
    max_padding: int = 6
    initial_padding: int = 2
    delay_steps: int = 0
    padding_bonus: float = 0.0
    max_entries: int = 256
    max_tokens: int = 2048
    max_prefix: int = 0

    def to_c(self) -> "_capi.TTSParams":
        p = _capi.TTSParams()
        p.text_card, p.new_word, p.pad, p.zero = int(self.text_card), int(self.new_word), int(self.pad), int(self.zero)
        p.second_stream_ahead, p.max_padding = int(self.second_stream_ahead), int(self.max_padding)
        p.initial_padding, p.delay_steps = int(self.initial_padding), int(self.delay_steps)
        p.padding_bonus = float(self.padding_bonus)
        return p


@dataclass
class TTSScript:
    """One session's script: `entries` = [(tokens, padding), ...] (the reference's `Entry.tokens` / `Entry.padding`; no tokens =
    a break), and optionally the rows of `generate(prefixes=...)`: `text_prefix` [T] and `audio_prefix` [dep_q, T], un-delayed
    (-2 = leave the sampled token)."""
    entries: Sequence = field(default_factory=list)
    text_prefix: Optional[Sequence[int]] = None
    audio_prefix: Optional[Sequence[Sequence[int]]] = None


@dataclass
class TTSScriptStatus:
    """`TTSResult.end_steps[b]` (None while the script has not run out) and `all_consumption_times[b]` of one session."""
    has_script: bool
    end_step: Optional[int]
    n_consumed: int
    consumption_times: list


def _apply_nucleus(lib, handle, top_p: float, top_p_text: float, session_top_p: bool) -> bool:
    """The handle's nucleus settings for the stream about to start (the handle is shared by every LMGen / SessionBatcher built on the
    model, so each start states them).  Returns whether the stream runs the nucleus samplers."""
    on = top_p > 0 or top_p_text > 0 or session_top_p
    if on:
        lib.check(lib.mmi_lm_enable_nucleus(handle, 1))
        lib.check(lib.mmi_lm_set_top_p(handle, float(top_p), float(top_p_text)))
    elif hasattr(lib.cdll, "mmi_lm_enable_nucleus"):       # (an older build of the engine has no nucleus to switch off)
        lib.check(lib.mmi_lm_set_top_p(handle, 0.0, 0.0))
        lib.check(lib.mmi_lm_enable_nucleus(handle, 0))
    return on


class LMGen:
    """Streaming generation (reference: lm.py:556-850), including classifier-free guidance (`cfg_coef`,
    `cfg_is_masked_until`, `cfg_is_no_text`), `sum` condition tensors through `lm_model.fuser` and the per-step hooks
    `on_text_logits_hook` / `on_text_hook` / `on_audio_hook` (the step then runs in segments with the callbacks in between,
    mmi_lm_set_hooks), and `cross` condition tensors for models built with cross-attention layers."""

    def __init__(self, lm_model: LMModel, use_sampling: bool = True, temp: float = 0.8, temp_text: float = 0.7,
                 top_k: int = 250, top_k_text: int = 25, cfg_coef: float = 1.0, check: bool = False,
                 condition_tensors=None, on_text_hook=None, on_text_logits_hook=None, on_audio_hook=None,
                 support_out_of_sync: bool = False, cfg_is_masked_until=None, cfg_is_no_text: bool = False,
                 seed: int = 0, tts_machine: Optional[TTSMachine] = None, top_p: float = 0.0, top_p_text: float = 0.0,
                 session_top_p: bool = False, logprobs: Optional[int] = None):
        assert not lm_model.training, "generation shouldn't be used in training mode."
        # log-probabilities of the stored tokens in the live step: None = off, n in 0..8 = on with n alternatives
        self.logprobs = None if logprobs is None else int(logprobs)
        # nucleus sampling (sampling.py:97-98: top_p > 0 overrides top_k): the stream runs the nucleus samplers iff a value is
        # positive or `session_top_p` asks for them (sessions then get their own values with `set_session_top_p`)
        check_top_p(top_p, top_p_text)
        self.top_p = float(top_p)
        self.top_p_text = float(top_p_text)
        self.session_top_p = bool(session_top_p)
        self._nucleus = False                             # the live stream runs the nucleus samplers
        if cfg_coef != 1.:                                # lm.py:600-603
            if not cfg_is_no_text and not cfg_is_masked_until:
                assert lm_model.fuser is not None, "Model has no fuser, cannot do CFG."
                assert condition_tensors, "Missing condition tensors for CFG."
        self.condition_tensors = condition_tensors
        self.cfg_is_masked_until = cfg_is_masked_until
        self.cfg_is_no_text = cfg_is_no_text
        # per-step hooks (lm.py:568-570, 734-757): each may modify its tensor in place, like the reference's
        self.on_text_hook = on_text_hook
        self.on_text_logits_hook = on_text_logits_hook
        self.on_audio_hook = on_audio_hook
        self._hooks_keep = None
        self._hook_error = None
        self.lm_model = lm_model
        self.use_sampling = use_sampling
        self.temp = temp
        self.temp_text = temp_text
        self.top_k = top_k
        self.top_k_text = top_k_text
        self.cfg_coef = cfg_coef
        self.check = check
        self.support_out_of_sync = support_out_of_sync
        self.max_delay = max(lm_model.delays)
        self.seed = seed
        # the reference's TTS state machine and generate()'s three hooks on the device; host hooks set next to it run after it
        self.tts_machine = tts_machine
        self._lib = lm_model._lib
        self._batch: Optional[int] = None

    # ---- plumbing ------------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self.lm_model.device

    def _stream(self):
        return _capi.stream_ptr(self.device)

    def _mask_ptr(self, mask: Optional[torch.Tensor]):
        if mask is None:
            return None, None
        m = mask.to(device=self.device, dtype=torch.bool).contiguous().view(torch.uint8)
        assert m.numel() == self._batch
        return m, m.data_ptr()

    # ---- streaming lifecycle -------------------------------------------------------------------
    @property
    def is_streaming(self) -> bool:
        return self._batch is not None

    def streaming_forever(self, batch_size: int) -> None:
        s = _capi.Sampling()
        s.use_sampling = 1 if self.use_sampling else 0
        s.temp, s.temp_text = self.temp, self.temp_text
        s.top_k, s.top_k_text = self.top_k, self.top_k_text
        s.seed = self.seed
        lm = self.lm_model
        g = _capi.Guidance()
        g.cfg_coef = float(self.cfg_coef)
        g.cfg_is_no_text = 1 if self.cfg_is_no_text else 0
        rows = int(batch_size) * (2 if self.cfg_coef != 1. else 1)
        keep = []
        if lm.fuser is None:                               # lm.py:616-628
            assert not self.condition_tensors
        else:
            assert self.condition_tensors is not None
            cs = lm.fuser.get_sum(self.condition_tensors)
            if cs is not None:
                assert cs.shape[0] == rows, "cfg requires 2x more conditions." if self.cfg_coef != 1. else "one condition row per session"
                cs = cs.to(device=self.device, dtype=torch.bfloat16).contiguous().view(rows, lm.dim)
                keep.append(cs)
                g.condition_sum = cs.data_ptr()
            cx = lm.fuser.get_cross(self.condition_tensors)                     # lm.py:623-627
            if cx is not None:
                assert cx.shape[0] == rows, "cfg requires 2x more conditions." if self.cfg_coef != 1. else "one condition row per session"
                cx = cx.to(device=self.device, dtype=torch.bfloat16).contiguous()
                assert cx.dim() == 3 and cx.shape[2] == lm.dim, cx.shape
                keep.append(cx)
                g.condition_cross = cx.data_ptr()
                g.cross_len = int(cx.shape[1])
        if lm.config.cross_attention:
            assert g.condition_cross, "the model has cross-attention layers: a `cross` condition tensor is required"   # transformer.py:793-795
        if self.cfg_is_masked_until is not None and self.cfg_coef != 1.:
            assert len(self.cfg_is_masked_until) == int(batch_size)
            mu = (C.c_int64 * int(batch_size))(*[int(v) for v in self.cfg_is_masked_until])
            keep.append(mu)
            g.cfg_is_masked_until = C.cast(mu, C.c_void_p)
        if self.tts_machine is not None:
            m = self.tts_machine
            self._lib.check(self._lib.mmi_lm_enable_tts_machine(lm._handle, C.byref(m.to_c()), int(m.max_entries), int(m.max_tokens),
                                                                int(m.max_prefix)))
        elif hasattr(self._lib.cdll, "mmi_lm_enable_tts_machine"):       # (an older build of the engine has no machine to switch off)
            self._lib.check(self._lib.mmi_lm_enable_tts_machine(lm._handle, None, 0, 0, 0))
        self._nucleus = _apply_nucleus(self._lib, lm._handle, self.top_p, self.top_p_text, self.session_top_p)
        _apply_logprobs(self._lib, lm._handle, self.logprobs)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        self._lib.check(self._lib.mmi_lm_streaming_start_guided(lm._handle, int(batch_size), C.byref(s), C.byref(g), self._stream()))
        del keep
        self._batch = int(batch_size)
        self._cond_keep = []
        self._install_hooks()

    def _install_hooks(self) -> None:
        """The reference calls `on_text_logits_hook(text_logits [B,1,1,card])`, `on_text_hook(text_token [B])` and
        `on_audio_hook(audio_tokens [B,dep_q])` between the stages of a step and lets them write in place (lm.py:734-757).
        Here each is a C callback of the segmented step: tensor out (mmi_lm_hook_io), Python hook, tensor back in - all
        stream-ordered, nothing synchronises."""
        lib, h = self._lib, self.lm_model._handle
        if not (self.on_text_logits_hook or self.on_text_hook or self.on_audio_hook):
            lib.check(lib.mmi_lm_set_hooks(h, None))
            self._hooks_keep = None
            return
        cfg, B = self.lm_model.config, self._batch

        def wrap(which, hook, make, view):
            if hook is None:
                return _capi.HOOK_FN()                      # NULL function pointer

            def cb(_user):
                try:
                    t = make()
                    lib.check(lib.mmi_lm_hook_io(h, which, 0, t.data_ptr(), t.numel() * t.element_size(), self._stream()))
                    hook(view(t))
                    lib.check(lib.mmi_lm_hook_io(h, which, 1, t.data_ptr(), t.numel() * t.element_size(), self._stream()))
                    return 0
                except BaseException as e:                  # never unwind through the C frames: report after the step
                    self._hook_error = e
                    return 1
            return _capi.HOOK_FN(cb)
        dev = self.device
        hooks = _capi.LMHooks()
        hooks.on_text_logits = wrap(0, self.on_text_logits_hook,
                                    lambda: torch.empty(B, cfg.text_card, device=dev, dtype=torch.bfloat16),
                                    lambda t: t.view(B, 1, 1, cfg.text_card))
        hooks.on_text_token = wrap(1, self.on_text_hook, lambda: torch.empty(B, device=dev, dtype=torch.int64), lambda t: t)
        hooks.on_audio_tokens = wrap(2, self.on_audio_hook, lambda: torch.empty(B, cfg.dep_q, device=dev, dtype=torch.int64),
                                     lambda t: t)
        self._hooks_keep = hooks                            # the callbacks must outlive the stream
        lib.check(lib.mmi_lm_set_hooks(h, C.byref(hooks)))

    def _stop_streaming(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._lib.mmi_lm_set_hooks(self.lm_model._handle, None)
        self._hooks_keep = None
        self._lib.check(self._lib.mmi_lm_streaming_stop(self.lm_model._handle))
        self._cond_keep = []
        self._batch = None

    @contextmanager
    def streaming(self, batch_size: int):
        self.streaming_forever(batch_size)
        try:
            yield self
        finally:
            self._stop_streaming()

    def reset_streaming(self, reset_mask: Optional[torch.Tensor] = None) -> None:
        assert self.is_streaming
        keep, ptr = self._mask_ptr(reset_mask)
        self._lib.check(self._lib.mmi_lm_reset(self.lm_model._handle, ptr, self._stream()))

    # ---- forking a session (mmi_lm_fork_session) ---------------------------------------------------
    def fork_session(self, src: int, dst) -> None:
        """Sessions `dst` (an int or a sequence of at most 16) become copies of session `src`: offset, KV ring, delay ring, last
        tokens, text history, sampling entry, top_p, condition and guidance coefficient, cross-attention source, TTS script
        position and adapter slot; what they held is gone as after `reset_streaming`, their exec bit is 1 whatever the source's
        is (a template parked under the exec mask stays parked), and their `last_logprobs()` read NaN / -1 until their next step.
        Stream-ordered, no host synchronisation; only the valid rows of the source's ring are moved.  A seeded `SessionSampling`
        continues with the same draws in the copy: set another afterwards for a different candidate.  No reference counterpart
        (the nearest: `get_streaming_state` / `set_streaming_state` on a batch of one).  With a `DuplexStream` call it after
        `join()`: the LM's own stream must have passed the last submitted frame."""
        assert self.is_streaming
        d = [int(dst)] if isinstance(dst, int) else [int(v) for v in dst]
        arr = (C.c_int32 * max(len(d), 1))(*d)
        self._lib.check(self._lib.mmi_lm_fork_session(self.lm_model._handle, int(src), arr, len(d), self._stream()))

    # ---- per-session sampling (mmi_lm_set_row_sampling) --------------------------------------------
    def _host_mask(self, mask):
        if mask is None:
            return None, None
        m = [1 if bool(v) else 0 for v in (mask.tolist() if isinstance(mask, torch.Tensor) else mask)]
        assert len(m) == self._batch
        arr = (C.c_uint8 * len(m))(*m)
        return arr, C.cast(arr, C.c_void_p)

    def set_session_sampling(self, settings, mask=None) -> None:
        """The masked sessions (all without a mask) sample with their own `SessionSampling` from the next step on: `settings` is
        one for all of them or a sequence with one per session.  Their text history (repetition penalty) starts empty.  Stream
        ordered; the launch list and a captured step graph stay as they are.  On a stream with the nucleus samplers the settings'
        `top_p` / `top_p_text` become the sessions' own as well - 0, the default, turns a session's nucleus OFF whatever this
        LMGen's `top_p` is; a session that should keep the stream's nucleus passes those values (or gets them back with
        `clear_session_top_p`)."""
        assert self.is_streaming
        if isinstance(settings, SessionSampling):
            settings = [settings] * self._batch
        assert len(settings) == self._batch, "one SessionSampling, or one per session"
        rows = (_capi.RowSampling * self._batch)(*[x.to_c() for x in settings])
        keep, ptr = self._host_mask(mask)
        # the nucleus part first, so that a refusal changes nothing: the domain, and a positive value on a stream without the samplers
        picked = [b for b in range(self._batch) if keep is None or keep[b]]
        for b in picked:
            check_top_p(settings[b].top_p, settings[b].top_p_text)
            if (settings[b].top_p > 0 or settings[b].top_p_text > 0) and not self._nucleus:
                raise RuntimeError("SessionSampling.top_p > 0 needs a stream with the nucleus samplers: LMGen(session_top_p=True)")
        self._lib.check(self._lib.mmi_lm_set_row_sampling(self.lm_model._handle, ptr, rows, self._stream()))
        if self._nucleus:
            for b in picked:
                self.set_session_top_p(b, settings[b].top_p, settings[b].top_p_text)

    def clear_session_sampling(self, mask=None) -> None:
        """The masked sessions (all without a mask) sample with this LMGen's own settings and counter again - its `top_p` /
        `top_p_text` included: on a stream with the nucleus samplers this also undoes a `set_session_top_p` of those sessions."""
        assert self.is_streaming
        keep, ptr = self._host_mask(mask)
        self._lib.check(self._lib.mmi_lm_clear_row_sampling(self.lm_model._handle, ptr, self._stream()))
        if self._nucleus:
            for b in range(self._batch):
                if keep is None or keep[b]:
                    self.clear_session_top_p(b)

    # ---- per-session nucleus (mmi_lm_set_row_top_p) ---------------------------------------------------
    def set_session_top_p(self, session: int, top_p: float, top_p_text: float) -> None:
        """Session `session` samples with its own nucleus values from the next step on (0 = off for that session: its top_k).
        Needs a stream with the nucleus samplers (`top_p` / `top_p_text` > 0 or `session_top_p=True`).  Stream-ordered; the launch
        list and a captured step graph stay as they are, and no other session changes.  `reset_streaming` keeps it."""
        assert self.is_streaming
        self._lib.check(self._lib.mmi_lm_set_row_top_p(self.lm_model._handle, int(session), float(top_p), float(top_p_text), self._stream()))

    def clear_session_top_p(self, session: int) -> None:
        """Session `session` returns to this LMGen's own `top_p` / `top_p_text`."""
        assert self.is_streaming
        self._lib.check(self._lib.mmi_lm_clear_row_top_p(self.lm_model._handle, int(session), self._stream()))

    # ---- per-session conditions (mmi_lm_set_row_condition) ---------------------------------------
    def set_session_condition(self, session: int, cond: SessionCondition) -> None:
        """Session `session` runs with its own condition (sum row, cross-attention source of its own length) and guidance
        coefficient from the next step on.  Stream-ordered; the launch list and a captured step graph stay as they are, and no other
        session changes.  `reset_streaming` keeps it.  With a `DuplexStream` call it after `join()`: the LM's own stream must have
        passed the last submitted frame."""
        assert self.is_streaming
        lm = self.lm_model
        rows = 2 if self.cfg_coef != 1. else 1
        rc = _capi.RowCondition()
        rc.cfg_coef = float(cond.cfg_coef)
        keep = []
        if cond.condition_tensors is not None:
            assert lm.fuser is not None, "Model has no fuser"
            cs = lm.fuser.get_sum(cond.condition_tensors)
            if cs is not None:
                assert cs.shape[0] == rows, "cfg requires 2x more conditions." if rows == 2 else "one condition row per session"
                cs = cs.to(device=self.device, dtype=torch.bfloat16).contiguous().view(rows, lm.dim)
                keep.append(cs)
                rc.condition_sum = cs.data_ptr()
            cx = lm.fuser.get_cross(cond.condition_tensors)
            if cx is not None:
                assert cx.shape[0] == rows, "cfg requires 2x more conditions." if rows == 2 else "one condition row per session"
                cx = cx.to(device=self.device, dtype=torch.bfloat16).contiguous()
                assert cx.dim() == 3 and cx.shape[2] == lm.dim, cx.shape
                keep.append(cx)
                rc.condition_cross = cx.data_ptr()
                rc.cross_len = int(cx.shape[1])
        self._lib.check(self._lib.mmi_lm_set_row_condition(lm._handle, int(session), C.byref(rc), self._stream()))
        self._cond_keep.append(keep)         # alive until the next step has been enqueued behind the call

    # ---- per-session adapters (mmi_lm_set_row_adapter) ------------------------------------------------
    def set_session_adapter(self, session: int, slot: Optional[int]) -> None:
        """Session `session` (both model rows of a guided one) runs on adapter `slot` of `LMModel(adapters=...)` from the next step
        on; None = the base model alone.  Stream-ordered; the launch list and a captured step graph stay as they are, and no other
        session changes.  `reset_streaming` keeps it; `streaming()` starts every session without an adapter."""
        assert self.is_streaming
        self._lib.check(self._lib.mmi_lm_set_row_adapter(self.lm_model._handle, int(session), -1 if slot is None else int(slot), self._stream()))

    def session_adapter(self, session: int) -> Optional[int]:
        """The adapter slot session `session` runs on, or None."""
        assert self.is_streaming
        slot = int(self._lib.mmi_lm_row_adapter(self.lm_model._handle, int(session)))
        return None if slot < 0 else slot

    # ---- per-session TTS scripts (mmi_lm_set_row_script) ---------------------------------------------
    def set_session_script(self, session: int, script: Optional[TTSScript]) -> None:
        """Session `session` runs `script` from its start from the next step on (None: no script, its sampled text token passes
        through).  Needs `LMGen(tts_machine=...)`.  Stream-ordered; the launch list and a captured step graph stay as they are,
        and no other session changes.  `reset_streaming` rewinds the session to the start of the same script."""
        assert self.is_streaming
        h = self.lm_model._handle
        if script is None:
            self._lib.check(self._lib.mmi_lm_set_row_script(h, int(session), None, self._stream()))
            return
        toks, first, pads = [], [0], []
        for tokens, padding in script.entries:
            toks.extend(int(t) for t in tokens)
            first.append(len(toks))
            pads.append(int(padding))
        arr = lambda v: (C.c_int32 * max(len(v), 1))(*v)
        sc = _capi.TTSScriptC()
        keep = [arr(toks), arr(first), arr(pads)]
        sc.tokens, sc.entry_first, sc.entry_padding = (C.cast(k, C.POINTER(C.c_int32)) for k in keep)
        sc.n_entries = len(pads)
        if script.text_prefix is not None:
            tp = [int(v) for v in (script.text_prefix.tolist() if isinstance(script.text_prefix, torch.Tensor) else script.text_prefix)]
            keep.append(arr(tp))
            sc.text_prefix, sc.text_prefix_len = C.cast(keep[-1], C.POINTER(C.c_int32)), len(tp)
        if script.audio_prefix is not None:
            ap = torch.as_tensor(script.audio_prefix, dtype=torch.int64).cpu()
            assert ap.dim() == 2 and ap.shape[0] == self.lm_model.dep_q, "audio_prefix must be [dep_q, T]"
            keep.append(arr([int(v) for v in ap.reshape(-1).tolist()]))
            sc.audio_prefix, sc.audio_prefix_len = C.cast(keep[-1], C.POINTER(C.c_int32)), int(ap.shape[1])
        self._lib.check(self._lib.mmi_lm_set_row_script(h, int(session), C.byref(sc), self._stream()))     # the call copies the arrays

    def session_script_status(self, session: int) -> TTSScriptStatus:
        """Where session `session`'s script stands (waits for the steps enqueued so far)."""
        assert self.is_streaming
        cap = int(self.tts_machine.max_entries) if self.tts_machine is not None else 0
        times = (C.c_int32 * max(cap, 1))()
        st = _capi.TTSStatus()
        st.consumption_times, st.capacity = C.cast(times, C.POINTER(C.c_int32)), cap
        self._lib.check(self._lib.mmi_lm_row_script_status(self.lm_model._handle, int(session), C.byref(st), self._stream()))
        return TTSScriptStatus(bool(st.has_script), None if st.end_step < 0 else int(st.end_step), int(st.n_consumed),
                               [int(times[i]) for i in range(min(st.n_consumed, cap))])

    def get_streaming_state(self) -> dict:
        """streaming.py:158-166: the complete streaming state (a copy: one opaque device tensor + the host step counter)."""
        assert self.is_streaming
        h = self.lm_model._handle
        n = int(self._lib.mmi_lm_state_bytes(h))
        buf = torch.empty(n, dtype=torch.uint8, device=self.device)
        word = C.c_int64(0)
        self._lib.check(self._lib.mmi_lm_state_save(h, buf.data_ptr(), n, C.byref(word), self._stream()))
        return {"lm_gen": buf, "offset_cpu": int(word.value), "batch_size": self._batch}

    def set_streaming_state(self, state: dict) -> None:
        """streaming.py:168-181."""
        assert self.is_streaming
        if "lm_gen" not in state:
            raise RuntimeError("Expected to find a streaming state for lm_gen.")
        buf = state["lm_gen"]
        self._lib.check(self._lib.mmi_lm_state_load(self.lm_model._handle, buf.data_ptr(), buf.numel(), int(state["offset_cpu"]), self._stream()))

    def set_streaming_detached(self, streaming_detached: bool) -> None:
        """streaming.py:78-86 (lm.py:579 calls it on the model): see LMModel.set_streaming_detached."""
        self._streaming_detached = bool(streaming_detached)

    def set_exec_mask(self, exec_mask: torch.Tensor) -> None:
        assert self.is_streaming
        keep, ptr = self._mask_ptr(exec_mask)
        self._lib.check(self._lib.mmi_lm_set_exec_mask(self.lm_model._handle, ptr, self._stream()))

    # ---- test / benchmark aids (no reference counterpart) -----------------------------------------
    def seek(self, offsets) -> None:
        """Move every session to stream position offsets[b] without touching the KV ring (mmi_lm_seek): the skipped positions
        read whatever the ring holds (zeros after `streaming`).  For ring-wrap tests at the real capacity and for timing a
        full-context step without thousands of warm-up steps."""
        assert self.is_streaming
        offs = [int(v) for v in offsets]
        assert len(offs) == self._batch
        arr = (C.c_int64 * len(offs))(*offs)
        self._lib.check(self._lib.mmi_lm_seek(self.lm_model._handle, C.cast(arr, C.c_void_p), self._stream()))

    def kv_ring(self, layer: int, which: str = "k") -> torch.Tensor:
        """Test aid (`mmi_lm_debug_kv_ring`): the raw bytes of temporal layer `layer`'s key ("k") or value ("v") ring, a uint8 copy.
        bf16 ring: [rows, H, cap, Dh] bf16 as bytes; "fp8": the same in e4m3 bytes; "fp4": the codes plane [rows, H, cap, Dh/2]
        followed by the scale plane [rows, H, cap, Dh/16] (rows = model rows: sessions, then their guidance twins)."""
        assert self.is_streaming
        h = self.lm_model._handle
        n = int(self._lib.mmi_lm_debug_kv_ring(h, int(layer), {"k": 0, "v": 1}[which], None, 0, self._stream()))
        if n < 0:
            self._lib.check(n)
        buf = torch.empty(n, dtype=torch.uint8, device=self.device)
        got = int(self._lib.mmi_lm_debug_kv_ring(h, int(layer), {"k": 0, "v": 1}[which], buf.data_ptr(), n, self._stream()))
        if got < 0:
            self._lib.check(got)
        return buf

    def state_regions(self) -> dict:
        """Test aid (`mmi_lm_debug_state_regions`): {name: (offset, bytes, rows, kind)} - where each part of the streaming state sits
        in `get_streaming_state()["lm_gen"]`; rows > 0: that many equal per-session slices; kind 1 = state, 0 = per-step scratch."""
        assert self.is_streaming
        text = _capi.read_text(lambda buf, cap: self._lib.mmi_lm_debug_state_regions(self.lm_model._handle, buf, cap))
        out = {}
        for line in text.splitlines():
            name, off, nbytes, rows, kind = line.split("\t")
            out[name] = (int(off), int(nbytes), int(rows), int(kind))
        return out

    def hidden_taps(self) -> torch.Tensor:
        """Parity tap (tests): the residual stream of the LAST step after the first and after the last temporal layer, bf16
        [2, model rows, dim].  `lm_model.enable_hidden_taps()` must have been called before `streaming()`."""
        rows = self._lib.mmi_lm_model_rows(self.lm_model._handle)
        out = torch.empty(2, rows, self.lm_model.config.dim, device=self.device, dtype=torch.bfloat16)
        self._lib.check(self._lib.mmi_lm_get_hidden_taps(self.lm_model._handle, out.data_ptr(), out.numel() * 2, self._stream()))
        return out

    def launch_list(self, with_bytes: bool = False):
        """[(site, kernel)] per kernel launch of one step, in launch order (recorded during the first step); with_bytes: a
        third field, the weight bytes a GEMM launch streams."""
        return _capi.launch_list(lambda buf, cap: self._lib.mmi_lm_launch_list(self.lm_model._handle, buf, cap), with_bytes)

    # ---- step ------------------------------------------------------------------------------------
    def _step(self, input_tokens: torch.Tensor, want_taps: bool, noise: Optional[torch.Tensor],
              forced: Optional[torch.Tensor]):
        if not self.is_streaming:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        assert input_tokens.dim() == 3, "Shape should be [B, K, T]."
        B, Ki, S = input_tokens.shape
        assert B == self._batch, f"Got a batch size {B}, expected {self._batch}"
        assert S == 1, "Only support being given steps one by one."
        cfg = self.lm_model.config
        needed = cfg.n_q - cfg.dep_q
        assert Ki >= needed, f"We expect {needed} tokens from the user stream, got {Ki}."
        codes = input_tokens.to(device=self.device, dtype=torch.int64).contiguous()
        if self.check:
            # lm.py:703-711 asserts on the model's input after the delay ring; the only values that enter that ring from outside
            # are these user codes (the rest the engine samples itself), so the same two conditions are asserted on them here -
            # like the reference's, a host synchronisation that only a debugging run pays
            user = codes[:, :needed]
            assert not (user == self.lm_model.ungenerated_token_id).any(), user
            assert (user <= self.lm_model.card).all(), user
        out = torch.empty(B, cfg.dep_q + 1, 1, device=self.device, dtype=torch.int64)
        tl = al = None
        tlp = alp = None
        if want_taps:
            tl = torch.empty(B, cfg.text_card, device=self.device, dtype=torch.float32)
            al = torch.empty(B, cfg.dep_q, cfg.card, device=self.device, dtype=torch.float32)
            tlp, alp = tl.data_ptr(), al.data_ptr()
        npz = None
        if noise is not None:
            kmax = max(self.top_k, self.top_k_text, 1)
            noise = noise.to(device=self.device, dtype=torch.float32).contiguous()
            assert noise.shape == (B, 1 + cfg.dep_q, kmax), f"noise must be [B, 1+dep_q, {kmax}]"
            npz = noise.data_ptr()
        if forced is not None:
            f = forced.to(device=self.device, dtype=torch.int64).contiguous().view(B, 1 + cfg.dep_q)
            self._lib.check(self._lib.mmi_lm_force_next_tokens(self.lm_model._handle, f.data_ptr(), self._stream()))
        valid = C.c_int32(0)
        self._hook_error = None
        rc = self._lib.mmi_lm_step(self.lm_model._handle, codes.data_ptr(), Ki, out.data_ptr(), tlp, alp, npz, B,
                                   C.byref(valid), self._stream())
        if rc and self._hook_error is not None:             # a Python hook raised: surface ITS exception
            err, self._hook_error = self._hook_error, None
            raise err
        self._lib.check(rc)
        self._cond_keep = []
        if not self.support_out_of_sync and not valid.value:
            return None, tl, al
        return out, tl, al

    @torch.no_grad()
    def prefill(self, input_tokens: torch.Tensor, forced_tokens: torch.Tensor, sessions: Optional[Sequence[int]] = None) -> None:
        """Known frames into live sessions without stepping them (mmi_lm_prefill; needs `LMModel(prefill_rows=)`): `input_tokens`
        [n, n_q - dep_q, T] int64 user codes and `forced_tokens` [n, 1 + dep_q, T] int64 (text, then the audio codebooks: what each
        frame's step would have stored, e.g. a log of `last_tokens()`) for the `n` sessions `sessions` (default: all of them).  The
        sessions end where T forced steps under an exec mask of exactly them would have left them - offsets, delay ring, text
        history, layer-0 K/V bit for bit, deeper K/V up to attention summation order - but nothing is sampled or returned, the other
        sessions are untouched and the stream's draw counter stays.  Stream ordered."""
        if not self.is_streaming:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        cfg = self.lm_model.config
        needed = cfg.n_q - cfg.dep_q
        sess = list(range(self._batch)) if sessions is None else [int(b) for b in sessions]
        n = len(sess)
        assert forced_tokens.dim() == 3 and input_tokens.dim() == 3, "Shape should be [n, K, T]."
        T = int(forced_tokens.shape[2])
        assert forced_tokens.shape[0] == n and input_tokens.shape[0] == n, f"one row of frames per session: got {forced_tokens.shape[0]} for {n}"
        assert forced_tokens.shape[1] == 1 + cfg.dep_q, f"forced_tokens must be [n, {1 + cfg.dep_q}, T]"
        assert input_tokens.shape[1] >= needed and input_tokens.shape[2] == T, f"We expect {needed} tokens from the user stream for each of the {T} frames."
        codes = input_tokens[:, :needed].to(device=self.device, dtype=torch.int64).contiguous()
        forced = forced_tokens.to(device=self.device, dtype=torch.int64).contiguous()
        if self.check:
            assert not (codes == self.lm_model.ungenerated_token_id).any(), codes
            assert (codes <= self.lm_model.card).all(), codes
            assert (forced >= 0).all(), f"forced_tokens must be >= 0: {forced}"
        arr = (C.c_int32 * max(n, 1))(*sess)
        self._lib.check(self._lib.mmi_lm_prefill(self.lm_model._handle, arr, n, codes.data_ptr() if needed else None, forced.data_ptr(), T,
                                                 self._stream()))
        self._cond_keep = []
        if self.device.type == "cuda":       # the launches read `codes` / `forced`: keep them until they ran
            codes.record_stream(torch.cuda.current_stream(self.device))
            forced.record_stream(torch.cuda.current_stream(self.device))

    @torch.no_grad()
    def score(self, input_tokens: torch.Tensor, tokens: torch.Tensor, sessions: Optional[Sequence[int]] = None, commit: bool = True,
              return_logits: bool = False) -> "ScoreOutput":
        """Teacher-forced scoring of known frames (mmi_lm_score; needs `LMModel(prefill_rows=, score=True)`): the model's
        distribution over tokens that are already known, the engine's counterpart of `LMModel.forward` (lm.py:322-377, 410-448) on a
        live session.  `input_tokens` [n, n_q - dep_q, T] and `tokens` [n, 1 + dep_q, T] int64 are `prefill`'s arguments; for every
        (session, site, frame) - site 0 the text head, then the `dep_q` audio heads - the result holds what the forced step of that
        frame computes: `logp`, the natural log of softmax(logits)[given token] (-inf where the token lies outside the head's range),
        `argmax`, and with `return_logits` the raw logits.  Sampling settings play no part.
        `commit=True`: the sessions end exactly where `prefill` of the same arguments leaves them.  `commit=False`: nothing of the
        streaming state changes (pure rescoring of candidates against a live session); n * T must fit one pass (`prefill_rows`).
        Either way the other sessions and the stream's draw counter are untouched.  Stream ordered."""
        if not self.is_streaming:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        if not self.lm_model.score:
            raise RuntimeError("score is not enabled: build the model with LMModel(..., prefill_rows=N, score=True)")
        cfg = self.lm_model.config
        needed = cfg.n_q - cfg.dep_q
        sess = list(range(self._batch)) if sessions is None else [int(b) for b in sessions]
        n = len(sess)
        assert tokens.dim() == 3 and input_tokens.dim() == 3, "Shape should be [n, K, T]."
        T = int(tokens.shape[2])
        assert tokens.shape[0] == n and input_tokens.shape[0] == n, f"one row of frames per session: got {tokens.shape[0]} for {n}"
        assert tokens.shape[1] == 1 + cfg.dep_q, f"tokens must be [n, {1 + cfg.dep_q}, T]"
        assert input_tokens.shape[1] >= needed and input_tokens.shape[2] == T, f"We expect {needed} tokens from the user stream for each of the {T} frames."
        codes = input_tokens[:, :needed].to(device=self.device, dtype=torch.int64).contiguous()
        given = tokens.to(device=self.device, dtype=torch.int64).contiguous()
        if self.check:
            assert not (codes == self.lm_model.ungenerated_token_id).any(), codes
            assert (codes <= self.lm_model.card).all(), codes
            assert (given >= 0).all(), f"tokens must be >= 0: {given}"
        sites = 1 + cfg.dep_q
        logp = torch.empty(n, T, sites, dtype=torch.float32, device=self.device)
        argmax = torch.empty(n, T, sites, dtype=torch.int32, device=self.device)
        tl = al = None
        if return_logits:
            tl = torch.empty(n, T, cfg.text_card, dtype=torch.float32, device=self.device)
            if cfg.dep_q:
                al = torch.empty(n, T, cfg.dep_q, cfg.card, dtype=torch.float32, device=self.device)
        out = _capi.ScoreOut(logp.data_ptr(), argmax.data_ptr(), tl.data_ptr() if tl is not None else None,
                             al.data_ptr() if al is not None else None)
        arr = (C.c_int32 * max(n, 1))(*sess)
        self._lib.check(self._lib.mmi_lm_score(self.lm_model._handle, arr, n, codes.data_ptr() if needed else None, given.data_ptr(), T,
                                               1 if commit else 0, C.byref(out), self._stream()))
        if commit:
            self._cond_keep = []
        if self.device.type == "cuda":       # the launches read `codes` / `given`: keep them until they ran
            codes.record_stream(torch.cuda.current_stream(self.device))
            given.record_stream(torch.cuda.current_stream(self.device))
        return ScoreOutput(logp.transpose(1, 2), argmax.transpose(1, 2).to(torch.int64), tl, al)

    def last_tokens(self) -> torch.Tensor:
        """[B, 1 + dep_q] int64: the tokens the last step (or prefill) stored for every session, in step coordinates - one frame of
        the log `prefill` takes back (`step`'s own return value lags by the delays)."""
        assert self.is_streaming
        out = torch.empty(self._batch, 1 + self.lm_model.dep_q, dtype=torch.int64, device=self.device)
        self._lib.check(self._lib.mmi_lm_last_tokens(self.lm_model._handle, out.data_ptr(), self._stream()))
        return out

    def _logprobs(self, call) -> LogProbs:
        assert self.is_streaming
        B, S, n = self._batch, 1 + self.lm_model.dep_q, self.logprobs or 0
        logp = torch.empty(B, S, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, S, n, dtype=torch.int32, device=self.device)
        tlp = torch.empty(B, S, n, dtype=torch.float32, device=self.device)
        self._lib.check(call(self.lm_model._handle, logp.data_ptr(), ids.data_ptr() if n else None, tlp.data_ptr() if n else None,
                             self._stream()))
        return LogProbs(logp, ids.to(torch.int64), tlp)

    def last_logprobs(self) -> LogProbs:
        """Step coordinates (`LMGen(logprobs=n)`): lines up with `last_tokens()`.  A session that did not execute keeps its last
        executed step's values; one that has not executed since the start or its reset reads NaN / -1."""
        return self._logprobs(self._lib.mmi_lm_last_logprobs)

    def frame_logprobs(self) -> LogProbs:
        """Frame coordinates: lines up with the frame the last `step` returned - NaN / -1 exactly where that frame holds -2
        (`step` then returned None for the batch, or the session did not execute)."""
        return self._logprobs(self._lib.mmi_lm_frame_logprobs)

    @torch.no_grad()
    def step(self, input_tokens: torch.Tensor, depformer_replace_tokens: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """[B, >= n_q - dep_q, 1] int64 user codes (8 for Moshi, none - [B, 0, 1] - for a TTS model where n_q == dep_q) ->
        [B, 1 + dep_q, 1] int64 (text + generated audio) or None during the delay."""
        forced = None
        if depformer_replace_tokens is not None:   # lm.py:751-755
            assert depformer_replace_tokens.dim() == 3
            B = depformer_replace_tokens.shape[0]
            forced = torch.full((B, 1 + self.lm_model.dep_q), -1, dtype=torch.int64, device=self.device)
            forced[:, 1:] = depformer_replace_tokens.to(self.device).squeeze(-1)
        out, _, _ = self._step(input_tokens, False, None, forced)
        return out

    @torch.no_grad()
    def step_with_extra_heads(self, input_tokens: torch.Tensor, depformer_replace_tokens: Optional[torch.Tensor] = None):
        """lm.py:793-807: `step` plus softmax(extra_head(transformer_out)) for every extra head, each [model rows, 1, dim]."""
        out = self.step(input_tokens, depformer_replace_tokens)
        if out is None:
            return None
        cfg = self.lm_model.config
        rows = int(self._lib.mmi_lm_model_rows(self.lm_model._handle))
        probs = torch.empty(rows, max(cfg.extra_heads_num_heads, 1), cfg.extra_heads_dim, device=self.device, dtype=torch.float32)
        self._lib.check(self._lib.mmi_lm_extra_heads(self.lm_model._handle, probs.data_ptr(), self._stream()))
        heads = [probs[:, h][:, None].to(torch.bfloat16) for h in range(cfg.extra_heads_num_heads)]
        return out, heads

    @torch.no_grad()
    def step_with_taps(self, input_tokens: torch.Tensor, noise: Optional[torch.Tensor] = None,
                       forced_tokens: Optional[torch.Tensor] = None
                       ) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
        """`step` plus the parity taps: text logits [B, text_card] and audio logits [B, dep_q, card] (fp32 copies of
        the bf16 logits the tokens were sampled from); `noise` replaces the RNG, `forced_tokens` teacher-forces."""
        return self._step(input_tokens, True, noise, forced_tokens)
