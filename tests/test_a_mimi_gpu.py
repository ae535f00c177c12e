"""Parity of the gfx950 Mimi engine on a real MI355X: golden vectors from the reference, the numpy oracle on
seeded inputs, and size-independent properties at the benchmark's batch sizes."""
import numpy as np
import pytest
import torch

from moshi_amd import MimiConfig, MimiModel, tiny_mimi_config
from moshi_amd.weights import random_mimi_state_dict
from tests import mimi_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture()
def factory(gpu_lib):
    def make(sd, cfg, K, max_batch=32):
        return MimiModel(sd, cfg, device=DEV, max_batch=max_batch, num_codebooks=K)
    return make


def test_tiny_schedule_matches_reference_golden(factory):
    mimi_cases.check_tiny_against_golden(factory, DEV)


def test_full_size_matches_reference_golden(factory):
    mimi_cases.check_full_against_golden(factory, DEV)


@pytest.mark.parametrize("B", [1, 5])
def test_tiny_matches_oracle_with_masks_and_reset(factory, B):
    mimi_cases.oracle_vs_engine(factory, DEV, tiny_mimi_config(), seed=31 + B, B=B, F=8, K=5)


def test_full_size_matches_oracle(factory):
    mimi_cases.oracle_vs_engine(factory, DEV, MimiConfig(), seed=77, B=2, F=2, K=8, use_masks=True)


def test_full_size_c2_recipe_crosses_the_ring_wrap(factory):
    """8 streams, 200 frames, random exec masks, one mid-run reset - the 250-slot rings of the codec's
    transformers wrap at frame 126 (the state bench.py runs in, never parity-tested at full size before)."""
    import json
    from pathlib import Path
    # the engine runs the 8 streams; the numpy checker follows three of them (the always-executing row whose rings wrap at frame
    # 126, the nine-in-ten row (wraps ~140), the sine row, which is also reset mid-run) for 160 frames: ~85 s instead of 210 in a
    # suite with a time budget (four rows: 114 s on MI355X in round 5)
    res = mimi_cases.check_c2_recipe(factory, DEV, MimiConfig(), B=8, F=160, oracle_rows=[0, 1, 7])
    assert res["wrapped"]
    out = Path(__file__).resolve().parent.parent / "gpurun_out"
    if out.is_dir():
        (out / "parity_mimi_c2_recipe.json").write_text(json.dumps(res, indent=1))


def test_rvq_indices_bit_exact_on_many_vectors(factory):
    """131 072 index decisions (4096 latents x 32 levels) against the oracle's fp32 cdist restatement.
    The engine evaluates distances in fp64, i.e. it returns the exact nearest centroid; the fp32 reference formula
    can only disagree with that at a near-tie below its own resolution (relative gaps down to
    3e-6 occur about once in 1e5 decisions).  Any disagreement is therefore audited in fp64: it must be such a
    near-tie AND the engine must hold the exact argmin."""
    from oracle.mimi_oracle import MimiOracle
    cfg = MimiConfig()
    sd = random_mimi_state_dict(cfg, seed=1234)
    m = factory(sd, cfg, 32, max_batch=64)
    orc = MimiOracle(sd, cfg, num_codebooks=32)
    rng = np.random.default_rng(0)
    lat = rng.standard_normal((64, cfg.dimension, 64)).astype(np.float32)
    ce = m.quantize(torch.from_numpy(lat).to(DEV)).cpu().numpy()
    co = orc.quantize(lat)
    assert ce.shape == co.shape == (64, 32, 64)
    bad = np.argwhere((ce != co).any(1))
    # the observed count goes on record: printed, and written next to the other parity summaries
    n_dec = int((ce != co).sum())
    print(f"[parity] rvq_indices: {len(bad)} of 4096 vectors ({n_dec} of {ce.size} index decisions) differ from the fp32 cdist restatement")
    import json
    from pathlib import Path
    out = Path(__file__).resolve().parent.parent / "gpurun_out"
    if out.is_dir():
        (out / "parity_rvq_indices.json").write_text(json.dumps({"case": "rvq_indices", "vectors": 4096, "vectors_differing": len(bad),
                                                                  "decisions": int(ce.size), "decisions_differing": n_dec}, indent=1))
    assert len(bad) <= 4, f"{len(bad)} of 4096 vectors differ from the oracle - more than near-ties can explain"
    for b, t in bad:
        k = int(np.argmax(ce[b, :, t] != co[b, :, t]))          # first level that differs; the prefix is identical
        part = 0 if k < cfg.q_n_q_semantic else 1
        x = (orc.in_proj[part].astype(np.float64) @ lat[b, :, t].astype(np.float64)).astype(np.float32)
        k0 = 0 if part == 0 else cfg.q_n_q_semantic
        for kk in range(k0, k):
            x = (x - orc.codebooks[kk][co[b, kk, t]]).astype(np.float32)
        E = orc.codebooks[k].astype(np.float64)
        d = ((E - x.astype(np.float64)) ** 2).sum(-1)
        de, do = d[ce[b, k, t]], d[co[b, k, t]]
        assert abs(de - do) <= 2e-5 * min(de, do), f"not a near-tie: {de} vs {do}"
        assert de <= do, "the engine must hold the exact (fp64) nearest centroid"


def test_batch_rows_are_independent_and_graph_equals_eager(factory, monkeypatch):
    """Size-independent properties at the benchmark batch (B=32): every row equals the same stream run alone at B=1,
    and the hipGraph replay equals the eager launch list."""
    cfg = MimiConfig()
    sd = random_mimi_state_dict(cfg, seed=1234)
    g = torch.Generator().manual_seed(9)
    x = (0.25 * torch.randn(32, 1, cfg.frame_size * 3, generator=g)).to(DEV)
    big = factory(sd, cfg, 8, max_batch=32)
    with big.streaming(32):
        codes = big.encode(x)
        pcm = big.decode(codes)
    for row in (0, 17, 31):
        one = factory(sd, cfg, 8, max_batch=1)
        with one.streaming(1):
            c1 = one.encode(x[row:row + 1])
            p1 = one.decode(c1)
        assert torch.equal(c1, codes[row:row + 1])
        assert torch.allclose(p1, pcm[row:row + 1], atol=2e-5, rtol=2e-5)
    monkeypatch.setenv("MMI_NO_GRAPH", "1")
    eager = factory(sd, cfg, 8, max_batch=32)
    with eager.streaming(32):
        c2 = eager.encode(x)
        p2 = eager.decode(c2)
    assert torch.equal(c2, codes) and torch.equal(p2, pcm)


@pytest.fixture(scope="module")
def full_sd():
    """The full-size codec's seed 1234 weights, made once for the module."""
    return random_mimi_state_dict(MimiConfig(), seed=1234)


def record_parity(case, res):
    """One `[parity]` line per case (the figures on record are in profiles/mimi_batch_classes/README.md)."""
    print(f"[parity] mimi {case}: {res['decisions_differing']} index decisions differ on {res['rows_executed']} executed checked rows "
          f"(rows {res['rows_checked']} of {res['batch']}, {res['frames']} frames); worst PCM error {res['worst_pcm_over_tol']:.3f} x tolerance")


def kernel_count(res, name):
    """Launches of kernel `name` (template arguments are not part of a launch list's names) in the encoder's and the decoder's program."""
    return [res["kernels"][which].get(name, 0) for which in ("encode", "decode")]


# The batch sizes at which `plan_conv` / `add_transformer` change the full-size program, and the rows the numpy checker follows:
# the first and the last session, and the sessions on both sides of every 32-column tile edge of the 25 Hz (2 columns per session)
# and 12.5 Hz (1 column) layers.  profiles/mimi_batch_classes/README.md has the tiling of every layer at each of them.
BATCH_CLASSES = {
    9: [0, 7, 8],                  # first batch whose 512-channel layers (16 columns per session) run k_conv_wide; 4.5 tiles
    23: [0, 15, 16, 22],           # 16-column layers enter the 32-session table rows (11.5 tiles), all others on the planner's rule
    33: [0, 15, 16, 31, 32],       # 32-session rows with a half tile; 3 subtiles at 25 Hz; the second 12.5 Hz subtile holds one column
    47: [0, 31, 32, 46],           # 16-column layers on the 64-session rows, the rest still on the 32-session rows
    49: [0, 32, 47, 48],           # every tabled layer on the 64-session rows; the fourth 25 Hz subtile holds 2 columns
    64: [0, 31, 32, 47, 48, 63],   # the C5 batch; exactly 128 columns at 25 Hz
    65: [0, 32, 63, 64],           # 130 columns at 25 Hz: the unpacked transformer program
    68: [0, 64, 67],               # the largest batch the index arithmetic takes
}


@pytest.fixture(scope="module")
def handle68(full_sd):
    """ONE full-size handle for all the batch classes: plans are rebuilt at every `streaming_start`, and nothing of the stream
    before may survive into the next."""
    held = []

    def make(sd, cfg, K):
        assert sd is full_sd and K == 8
        if not held:
            held.append(MimiModel(sd, cfg, device=DEV, max_batch=68, num_codebooks=K))
        return held[0]
    yield make
    held.clear()


@pytest.mark.parametrize("B", sorted(BATCH_CLASSES))
def test_full_size_matches_oracle_at_every_batch_class(gpu_lib, handle68, full_sd, B):
    """The released codec against the oracle wherever the batch size changes the program: three frames with exec masks and the
    mid-run reset; codes equal on the checked rows, PCM within the suite's tolerance."""
    res = mimi_cases.oracle_vs_engine(handle68, DEV, MimiConfig(), seed=1000 + B, B=B, F=3, K=8, oracle_rows=BATCH_CLASSES[B], sd=full_sd)
    record_parity(f"batch_class_B{B}", res)
    ln, norms = kernel_count(res, "k_gemm_f32_ln"), kernel_count(res, "k_layernorm_ct")
    if B <= 64:            # packed transformer: one k_layernorm_ct in front, every other norm inside k_gemm_f32_ln
        assert min(ln) > 0 and max(norms) <= 2, (ln, norms)
    else:                  # plain buffers: every norm its own launch, the linears on k_conv_wide
        assert max(ln) == 0 and min(norms) > 2, (ln, norms)


def test_full_size_refuses_69_sessions(gpu_lib, full_sd):
    """69 sessions x 1920 samples pass the kernels' 2^17 index range: refused by name, never computed."""
    m = MimiModel(full_sd, MimiConfig(), device=DEV, max_batch=69, num_codebooks=8)
    with pytest.raises(NotImplementedError, match="131072"):
        with m.streaming(69):
            m.encode(torch.zeros(69, 1, MimiConfig().frame_size, device=DEV))


def test_full_size_general_shape_fallbacks(factory, full_sd, monkeypatch):
    """The general-shape fallbacks of the launch mergers (one RVQ level per launch pair, pack launches, two commit launches, dense
    rows) at the released codec's widths: product paths for other codec shapes, forced by their test hooks."""
    for var in ("MMI_RVQ_NO_PAIR", "MMI_MIMI_PACK_LAUNCHES", "MMI_MIMI_TWO_COMMITS", "MMI_MIMI_NO_ALIGN"):
        monkeypatch.setenv(var, "1")
    res = mimi_cases.oracle_vs_engine(factory, DEV, MimiConfig(), seed=1105, B=5, F=3, K=8, oracle_rows=range(5), sd=full_sd)
    record_parity("general_shape_fallbacks_B5", res)


@pytest.mark.parametrize("two_pass", [False, True])
def test_full_size_attention_kernels_across_a_ring_wrap(factory, full_sd, monkeypatch, two_pass):
    """Head dim 64 with a 10-slot ring and 16 positions: the one-round-trip kernel at a capacity other than 250, and the two-pass
    kernel behind its hook, both past the wrap."""
    from dataclasses import replace
    if two_pass:
        monkeypatch.setenv("MMI_MIMI_ATTN_TWO_PASS", "1")
    cfg = replace(MimiConfig(), tr_context=10)
    res = mimi_cases.oracle_vs_engine(factory, DEV, cfg, seed=1203, B=3, F=8, K=8, oracle_rows=range(3), sd=full_sd)
    record_parity(f"attention_ring_wrap_{'two_pass' if two_pass else 'one_pass'}", res)
    one, two = kernel_count(res, "k_mimi_attn_1pass"), kernel_count(res, "k_mimi_attn")
    assert (min(two) > 0 and max(one) == 0) if two_pass else (min(one) > 0 and max(two) == 0), res["kernels"]


def test_full_size_long_context_selects_the_two_pass_attention(factory, full_sd):
    """300 ring slots at head dim 64 are more than a thread's 16 row slots cover (256): the product picks k_mimi_attn itself."""
    from dataclasses import replace
    cfg = replace(MimiConfig(), tr_context=300)
    res = mimi_cases.oracle_vs_engine(factory, DEV, cfg, seed=1302, B=2, F=3, K=8, oracle_rows=range(2), sd=full_sd)
    record_parity("attention_context_300", res)
    assert min(kernel_count(res, "k_mimi_attn")) > 0 and max(kernel_count(res, "k_mimi_attn_1pass")) == 0, res["kernels"]


@pytest.mark.parametrize("mtb,w,ks", [(1, 2, 2), (2, 4, 3), (4, 8, 8), (4, 1, 1)])
def test_full_size_forced_tilings(gpu_lib, full_sd, monkeypatch, mtb, w, ks):
    """Every tiling the table may be retuned to, forced on every full-size layer at 33 sessions (a half tile on the 512-channel
    layers, a third 25 Hz subtile of 2 columns, a second 12.5 Hz subtile of one)."""
    monkeypatch.setenv("MMI_CONV_MTB", str(mtb))
    monkeypatch.setenv("MMI_CONV_W", str(w))
    monkeypatch.setenv("MMI_CONV_KSPLIT", str(ks))

    def make(sd, cfg, K):
        return MimiModel(sd, cfg, device=DEV, max_batch=33, num_codebooks=K)
    res = mimi_cases.oracle_vs_engine(make, DEV, MimiConfig(), seed=1433, B=33, F=2, K=8, oracle_rows=[0, 31, 32], sd=full_sd)
    record_parity(f"forced_tiling_mtb{mtb}_w{w}_ks{ks}_B33", res)


@pytest.mark.parametrize("B", [8, 32, 64, 68])
def test_codec_is_bit_reproducible_between_streams(factory, B):
    """The full-size codec at the C2 batch (8 streams), the benchmark batches (32, 64) and the largest one (68: the unpacked
    transformer program): three frames encoded and decoded, then four
    more streams on the SAME handle fed the same PCM - codes and PCM bit for bit equal to the first stream's (a launch that is not
    a function of its inputs - round 4's LM failure - is the one bug class a tolerance against the checker cannot see)."""
    cfg = MimiConfig()
    sd = random_mimi_state_dict(cfg, seed=1234)
    g = torch.Generator().manual_seed(19 + B)
    x = (0.25 * torch.randn(B, 1, cfg.frame_size * 3, generator=g)).to(DEV)
    m = factory(sd, cfg, 8, max_batch=B)

    def run():
        out = []
        with m.streaming(B):
            for f in range(3):
                codes = m.encode(x[:, :, f * cfg.frame_size:(f + 1) * cfg.frame_size])
                out.append((codes.clone(), m.decode(codes).clone()))
        return out
    first = run()
    for r in range(4):
        for f, ((c0, p0), (c1, p1)) in enumerate(zip(first, run())):
            assert torch.equal(c0, c1), f"repeat {r} frame {f}: codes differ between two streams fed the same PCM"
            assert torch.equal(p0, p1), f"repeat {r} frame {f}: PCM differs between two streams fed the same PCM"


def test_round_trip_sine_c1(factory):
    """BASELINE.json configs[0] restated: 1 s 440 Hz sine, streaming == non-streaming codes, PCM shape."""
    cfg = MimiConfig()
    m = factory(random_mimi_state_dict(cfg, seed=1234), cfg, 8, max_batch=1)
    t = torch.arange(24000) / 24000.0
    wav = (0.5 * torch.sin(2 * torch.pi * 440.0 * t)).view(1, 1, -1).to(DEV)
    codes = m.encode(wav)                       # pads to 13 frames
    assert codes.shape == (1, 8, 13) and codes.dtype == torch.int64
    with m.streaming(1):
        cs = torch.cat([m.encode(wav[..., f * 1920:(f + 1) * 1920]) for f in range(12)], -1)
    assert torch.equal(cs, codes[..., :12])
    pcm = m.decode(codes)
    assert pcm.shape == (1, 1, 13 * 1920) and torch.isfinite(pcm).all()
