"""TTS-family LMs on the MI355X: the reference's runs (tests/golden/lm_tts.npz) and a 1.6B-shaped model with random weights,
modelled on the published TTS configuration (not verified against a real checkpoint): repeated streams bit-identical, and the
low-rank tables and the weight schedule against the same model written out in full."""
from dataclasses import replace

import pytest
import torch

from moshi_amd.config import LMConfig
from moshi_amd.lm import ConditionFuser, LMGen, LMModel
from moshi_amd.weights import random_lm_state_dict
from tests import tts_cases

pytestmark = pytest.mark.gpu


def tts_16b_config(**kw) -> LMConfig:
    c = LMConfig(dim=2048, num_heads=16, num_layers=16, hidden_scale=4.125, context=500, n_q=32, dep_q=32, card=2048, text_card=8000,
                 depformer_dim=1024, depformer_dim_feedforward=int(4.125 * 1024), depformer_num_heads=16, depformer_num_layers=4,
                 delays=[0] + [2] * 32, cross_attention=True, depformer_weights_per_step_schedule=list(range(8)) + [8] * 24,
                 depformer_low_rank_embeddings=128, demux_second_text_stream=True)
    return replace(c, **kw)


def _cross(cfg, B, Tc=16, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (0.5 * torch.randn(B, Tc, cfg.dim, generator=g, device="cuda")).to(torch.bfloat16)
    return {"x": (x, torch.ones(B, Tc, dtype=torch.bool, device="cuda"))}


def _run(lm, cfg, B, steps, use_sampling=True, taps=False, seed=3):
    conds = _cross(cfg, B) if cfg.cross_attention else None
    gen = LMGen(lm, use_sampling=use_sampling, support_out_of_sync=True, condition_tensors=conds, seed=seed)
    toks, tls, als = [], [], []
    with gen.streaming(B):
        for _ in range(steps):
            codes = torch.zeros(B, cfg.n_q - cfg.dep_q, 1, dtype=torch.int64, device="cuda")
            if taps:
                out, tl, al = gen.step_with_taps(codes)
                tls.append(tl.cpu()); als.append(al.cpu())
            else:
                out = gen.step(codes)
            toks.append(out.cpu())
    return torch.stack(toks), tls, als


@pytest.mark.parametrize("name", ["g", "h"])
def test_tts_golden_on_gpu(gpu_lib, name):
    tts_cases.check_tts_golden("cuda", gpu_lib, name)


def test_tts_16b_shape_repeated_streams_are_bit_identical(gpu_lib):
    cfg = tts_16b_config()
    sd = random_lm_state_dict(cfg, seed=7, device="cuda")
    fuser = ConditionFuser({"cross": ["x"]})
    for B in (1, 32):
        lm = LMModel(sd, cfg, device="cuda", max_batch=B, lib=gpu_lib, fuser=fuser)
        a, _, _ = _run(lm, cfg, B, 20)
        b, _, _ = _run(lm, cfg, B, 20)
        assert torch.equal(a, b), f"B={B}: two streams of the same seed differ"
        assert (a[:, :, 1:] < cfg.card).all() and (a[:, :, 1:] >= -2).all()
        del lm
    del sd
    torch.cuda.empty_cache()


def test_tts_16b_shape_schedule_and_low_rank_equal_the_written_out_model(gpu_lib):
    """The scheduled, low-rank model against the same model with every shared set copied out to its micro-step and the tables
    expanded in torch (fp32 matmul on the GPU, then bf16): the engine must compute the same function, bit for bit.  Demux and
    cross-attention off (a demuxed table runs out1 / out2 instead of the low-rank linear, lm_utils.py:106-116)."""
    cfg = tts_16b_config(demux_second_text_stream=False, cross_attention=False, num_layers=4)
    sd = random_lm_state_dict(cfg, seed=11, device="cuda")
    sched = cfg.depformer_weights_per_step_schedule
    full_cfg = replace(cfg, depformer_weights_per_step_schedule=None, depformer_low_rank_embeddings=None)
    full = {}
    for k, v in sd.items():
        if k.endswith(".low_rank.weight"):
            continue
        stem = k[: -len(".weight")]
        if stem + ".low_rank.weight" in sd:          # a low-rank table: bf16(E @ W^T), fp32 sums
            v = (v.float() @ sd[stem + ".low_rank.weight"].float().t()).to(torch.bfloat16)
        full[k] = v
    for k in list(full):
        for pat in ("depformer_in.", ".self_attn.in_projs.", ".self_attn.out_projs.", ".gating."):
            if pat in k and k.startswith(("depformer_in.", "depformer.layers.")):
                head, _, rest = k.partition(pat)
                idx, _, tail = rest.partition(".")
                if int(idx) == 0:
                    for step, w in enumerate(sched):
                        full[f"{head}{pat}{step}.{tail}"] = sd[f"{head}{pat}{w}.{tail}"]
    B = 4
    lm_a = LMModel(sd, cfg, device="cuda", max_batch=B, lib=gpu_lib)
    ta, tla, ala = _run(lm_a, cfg, B, 12, use_sampling=False, taps=True)
    del lm_a
    lm_b = LMModel(full, full_cfg, device="cuda", max_batch=B, lib=gpu_lib)
    tb, tlb, alb = _run(lm_b, full_cfg, B, 12, use_sampling=False, taps=True)
    del lm_b, sd, full
    torch.cuda.empty_cache()
    assert torch.equal(ta, tb)
    for s in range(len(tla)):
        assert torch.equal(tla[s], tlb[s]) and torch.equal(ala[s], alb[s]), f"step {s}: logits differ"
