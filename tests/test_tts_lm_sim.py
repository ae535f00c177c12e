"""TTS-family LMs on the kernel simulator: the engine against the reference's runs (tests/golden/lm_tts.npz), the loader's and the
engine's validation of the new options, and the seeded weights of the existing configurations left as they were."""
from dataclasses import replace

import pytest
import torch

from tests import tts_cases
from moshi_amd import loaders
from moshi_amd.config import tiny_lm_config, tiny_stt_config, tiny_tts_config
from moshi_amd.lm import LMModel
from moshi_amd.weights import lm_state_spec, random_lm_state_dict


def test_tts_shape_matches_reference_golden(sim_lib):
    """dep_q = n_q = 20 (the 32-row depformer attention), schedule, low rank, demuxed text with a muxing on_text_hook, replaced
    audio tokens, cross + sum conditions, cfg_coef 2 with cfg_is_no_text, exec masks and a partial reset."""
    tts_cases.check_tts_golden("cpu", sim_lib, "g")


def test_moshi_shape_with_schedule_and_low_rank_matches_reference_golden(sim_lib):
    tts_cases.check_tts_golden("cpu", sim_lib, "h")


def _kwargs(cfg):
    kw = cfg.reference_kwargs()
    kw.pop("causal")
    return kw


def test_loader_maps_and_validates_the_tts_options():
    kw = _kwargs(tiny_tts_config())
    cfg = loaders.lm_config_from_kwargs(kw)
    assert cfg.depformer_weights_per_step_schedule == list(range(6)) + [6] * 14
    assert cfg.depformer_low_rank_embeddings == 16 and cfg.demux_second_text_stream
    assert cfg.depformer_num_weights == 7
    moved = dict(kw)
    moved["demux_second_stream"] = moved.pop("demux_second_text_stream")        # loaders.py:395-396
    assert loaders.lm_config_from_kwargs(moved).demux_second_text_stream
    with pytest.raises(ValueError, match="entries"):
        loaders.lm_config_from_kwargs({**kw, "depformer_weights_per_step_schedule": [0, 1, 2]})
    with pytest.raises(ValueError, match="without gaps"):
        loaders.lm_config_from_kwargs({**kw, "depformer_weights_per_step_schedule": [0, 2] * 10})
    with pytest.raises(ValueError, match="multiple of 8"):
        loaders.lm_config_from_kwargs({**kw, "depformer_low_rank_embeddings": 12})
    # none of the keys appears for a model that does not set them (reference_kwargs of every existing config is unchanged)
    for c in (tiny_lm_config(), tiny_stt_config()):
        k = c.reference_kwargs()
        assert not {"depformer_weights_per_step_schedule", "depformer_low_rank_embeddings", "demux_second_text_stream"} & set(k)


def test_state_dict_layout_of_the_tts_options():
    cfg = tiny_tts_config()
    spec = {n: s for n, s, _ in lm_state_spec(cfg)}
    dd, r, N = cfg.depformer_dim, 16, cfg.text_card + 1
    assert [n for n in spec if n.startswith("depformer_in.")] == [f"depformer_in.{k}.weight" for k in range(7)]
    assert sum(n.startswith("linears.") for n in spec) == 20
    assert sum(".gating." in n and n.startswith("depformer.layers.0.") for n in spec) == 2 * 7
    assert spec["depformer_emb.3.weight"] == (cfg.card + 1, r) and spec["depformer_emb.3.low_rank.weight"] == (dd, r)
    assert spec["depformer_text_emb.weight"] == (N, r) and spec["depformer_text_emb.low_rank.weight"] == (dd, r)
    assert spec["depformer_text_emb.out1.weight"] == (dd, r) and spec["depformer_text_emb.out2.weight"] == (dd, r)
    assert spec["text_emb.out1.weight"] == (cfg.dim, cfg.dim) and spec["text_emb.out2.weight"] == (cfg.dim, cfg.dim)


# sha256 of random_lm_state_dict for the existing tiny configurations, taken before the TTS options existed: the committed
# goldens re-draw their weights from these seeds
DIGESTS = {
    ("tiny", 29): "77f63bf6c728353131671d37174d31da55b02950a9bd442ed8b5e2e05bf09678",
    ("stt", 37): "a5df95a79c5a508ba4a07bf4df6fd3f94b0ba68e567bbea8462a7f6196303077",
    ("cross", 53): "ad88308f990e05e878b1ad8f525684c42f24765727b5cdf0efc0cd77b96f0350",
}


def test_seeded_weights_of_existing_configs_are_unchanged():
    cfgs = {"tiny": tiny_lm_config(), "stt": tiny_stt_config(), "cross": replace(tiny_lm_config(), cross_attention=True)}
    for (name, seed), want in DIGESTS.items():
        assert tts_cases.state_dict_digest(random_lm_state_dict(cfgs[name], seed=seed)) == want, name


def test_quantised_linears_with_low_rank_or_demux_are_refused(sim_lib):
    cfg = tts_cases.h_config()
    sd = random_lm_state_dict(cfg, seed=3)
    with pytest.raises(NotImplementedError, match="low-rank or demuxed"):
        LMModel(sd, cfg, device="cpu", max_batch=2, lib=sim_lib, quantize=True)


def test_engine_refuses_a_schedule_with_a_gap(sim_lib):
    """The engine checks the schedule itself (a C caller of mmi_lm_create_ext has no loader in front of it)."""
    cfg = replace(tiny_lm_config(), depformer_weights_per_step_schedule=[0, 1, 1, 1, 1, 1, 1, 1])
    sd = random_lm_state_dict(cfg, seed=3)
    bad = replace(cfg, depformer_weights_per_step_schedule=[0, 2, 2, 2, 2, 2, 2, 2])
    with pytest.raises(Exception, match="no gaps"):
        LMModel(sd, bad, device="cpu", max_batch=2, lib=sim_lib)


def test_tts_model_steps_without_user_codes(sim_lib):
    """n_q == dep_q: LMGen.step takes [B, 0, 1] and returns [B, 1 + dep_q, 1]."""
    from moshi_amd.lm import LMGen
    cfg = replace(tiny_tts_config(), cross_attention=False)
    lm = LMModel(random_lm_state_dict(cfg, seed=5), cfg, device="cpu", max_batch=2, lib=sim_lib)
    gen = LMGen(lm, use_sampling=False, support_out_of_sync=True)
    with gen.streaming(2):
        for _ in range(3):
            out = gen.step(torch.zeros(2, 0, 1, dtype=torch.int64))
    assert out.shape == (2, 1 + cfg.dep_q, 1)
    assert (out[:, 1:] >= 0).all() and (out[:, 1:] < cfg.card).all()
