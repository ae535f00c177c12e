"""Parity cases shared by the simulator tests (CPU) and the GPU tests: engine vs golden vectors / oracle."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from moshi_amd import MimiConfig, MimiModel, tiny_mimi_config
from moshi_amd.weights import random_mimi_state_dict
from oracle.mimi_oracle import MimiOracle, cdist_argmin

GOLDEN = Path(__file__).resolve().parent / "golden"

# PCM tolerance: fp32 everywhere, only the summation order differs from the reference (MFMA k-order vs MKL/oneDNN).
# Stated as max |diff| <= PCM_ATOL + PCM_RTOL * max|ref| per frame.
PCM_ATOL, PCM_RTOL = 2e-5, 2e-5
LATENT_ATOL, LATENT_RTOL = 2e-5, 2e-5


def close(a: np.ndarray, b: np.ndarray, atol: float, rtol: float) -> bool:
    return float(np.abs(a - b).max()) <= atol + rtol * float(np.abs(b).max())


def load_tiny():
    g = np.load(GOLDEN / "mimi_tiny.npz")
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    return g, sd


def run_tiny_schedule(model_factory, device):
    """Replays the golden schedule (exec masks + partial reset) through an engine; returns per-frame outputs."""
    g, sd = load_tiny()
    cfg = tiny_mimi_config()
    K = int(g["num_codebooks"][0])
    m = model_factory(sd, cfg, K)
    x = torch.from_numpy(g["x"]).to(device)
    F, B = g["masks"].shape
    fs = cfg.frame_size
    lat, codes, pcm = [], [], []
    with m.streaming(B):
        for f in range(F):
            if f == int(g["reset_frame"][0]):
                m.reset_streaming(torch.from_numpy(g["reset_mask"]).to(device))
            m.set_exec_mask(torch.from_numpy(g["masks"][f]).to(device))
            xf = x[..., f * fs:(f + 1) * fs]
            c = m.encode(xf)
            # decode the REFERENCE codes so that a (legitimate) near-tie flip cannot cascade into the PCM check
            p = m.decode(torch.from_numpy(g["codes"][f]).to(device))
            codes.append(c.cpu().numpy()); pcm.append(p.cpu().numpy())
    return g, np.stack(codes), np.stack(pcm)


def check_tiny_against_golden(model_factory, device):
    g, codes, pcm = run_tiny_schedule(model_factory, device)
    masks = g["masks"]
    F, B = masks.shape
    for f in range(F):
        for b in range(B):
            if not masks[f, b]:
                continue        # rows that did not execute produce don't-care output (streaming.py:183-195)
            assert np.array_equal(codes[f, b], g["codes"][f, b]), f"codes differ at frame {f} row {b}"
            assert close(pcm[f, b], g["pcm"][f, b], PCM_ATOL, PCM_RTOL), f"pcm differs at frame {f} row {b}"


def check_full_against_golden(model_factory, device, frames=None):
    g = np.load(GOLDEN / "mimi_full.npz")
    cfg = MimiConfig()
    sd = random_mimi_state_dict(cfg, seed=int(g["seed"][0]))
    m = model_factory(sd, cfg, 8)
    x = torch.from_numpy(g["x"]).to(device)
    F = g["codes"].shape[0] if frames is None else frames
    B = x.shape[0]
    fs = cfg.frame_size
    with m.streaming(B):
        for f in range(F):
            xf = x[..., f * fs:(f + 1) * fs]
            lat = m.encode_to_latent(xf, quantize=False).cpu().numpy()
            assert close(lat, g["latent"][f], LATENT_ATOL, LATENT_RTOL), f"latent differs at frame {f}"
            c = m.quantize(torch.from_numpy(g["latent"][f]).to(device)).cpu().numpy()
            assert np.array_equal(c, g["codes"][f]), f"RVQ indices differ on the reference latent at frame {f}"
            p = m.decode(torch.from_numpy(g["codes"][f]).to(device)).cpu().numpy()
            assert close(p, g["pcm"][f], PCM_ATOL, PCM_RTOL), f"pcm differs at frame {f}"
    # end to end, the product call itself: encode(pcm) codes against the reference's codes, directly.  The
    # engine's latent differs from the reference's in the last bits (summation order), so an index may legitimately flip at a
    # near-tie of the reference's own distances: the match rate is printed and every mismatch audited on the golden latent.
    mism = []
    with m.streaming(B):
        for f in range(F):
            c = m.encode(x[..., f * fs:(f + 1) * fs]).cpu().numpy()
            for b, k, t in np.argwhere(c != g["codes"][f]):
                mism.append((f, int(b), int(k), int(t), int(c[b, k, t]), int(g["codes"][f][b, k, t])))
    total = F * int(np.prod(g["codes"][0].shape))
    print(f"[parity] mimi_full encode(pcm) vs reference codes: {total - len(mism)} of {total} index decisions equal")
    if mism:
        audit_code_mismatches(MimiOracle(sd, cfg, num_codebooks=8), [g["latent"][f] for f in range(F)], mism, max_vectors=1)
    return m


def audit_code_mismatches(orc, latents, mism, max_vectors, rel_gap=1e-4):
    """Every (frame, row, level, t, engine index, checker index) in `mism` must be a near-tie: at the checker's own residual
    (rebuilt from `latents[frame]`, the checker's un-quantised latent) the two candidates' squared distances, in fp64, differ
    by less than rel_gap - i.e. the decision is below what a last-bit difference of the latent can resolve - and only the
    FIRST differing level of a vector counts (later levels quantise a different residual).  At most `max_vectors` vectors."""
    firsts = {}
    for f, b, k, t, ce, co in mism:
        key = (f, b, t, 0 if k < orc.cfg.q_n_q_semantic else 1)
        if key not in firsts or k < firsts[key][0]:
            firsts[key] = (k, ce, co)
    assert len(firsts) <= max_vectors, f"{len(firsts)} vectors differ - more than near-ties explain: {sorted(firsts.items())[:5]}"
    for (f, b, t, part), (k, ce, co) in firsts.items():
        lat = latents[f]
        xr = (orc.in_proj[part].astype(np.float64) @ lat[b, :, t].astype(np.float64)).astype(np.float32)
        k0 = 0 if part == 0 else orc.cfg.q_n_q_semantic
        for kk in range(k0, k):
            idx = int(cdist_argmin(xr[None], orc.codebooks[kk])[0])
            xr = (xr - orc.codebooks[kk][idx]).astype(np.float32)
        E = orc.codebooks[k].astype(np.float64)
        d = ((E - xr.astype(np.float64)) ** 2).sum(-1)
        assert abs(d[ce] - d[co]) <= rel_gap * min(d[ce], d[co]), f"frame {f} row {b} level {k}: not a near-tie ({d[ce]} vs {d[co]})"


def oracle_vs_engine(model_factory, device, cfg, seed, B, F, K, use_masks=True, oracle_rows=None, sd=None):
    """Seeded comparison of an engine with the numpy oracle on identical inputs.
    oracle_rows (as in `check_c2_recipe`): the engine runs all B streams, the (slow, numpy) checker only these rows, with the masks
    and the reset sliced to them; the decoder is fed the checker's codes on the checked rows and the engine's own elsewhere.  The
    checked rows execute in the first and the last frame; every other mask bit stays random, so that masked-off neighbours
    inside a shared column tile still occur.  Codes on checked, executed rows equal the checker's: a difference must be ONE
    audited near-tie of the checker's own distances (`audit_code_mismatches`, max_vectors=1) in the whole run.  Without
    oracle_rows every row is checked and any differing code fails at once, with the random draws of every earlier caller.
    sd: a state dict made by the caller (the weights of `seed` otherwise).  Returns the worst PCM error as a multiple of the
    tolerance, the number of differing index decisions and the kernels of the two launch lists with their counts."""
    if sd is None:
        sd = random_mimi_state_dict(cfg, seed=seed)
    m = model_factory(sd, cfg, K)
    orc = MimiOracle(sd, cfg, num_codebooks=K)
    rng = np.random.default_rng(seed)
    x = (0.3 * rng.standard_normal((B, 1, cfg.frame_size * F))).astype(np.float32)
    rows = np.arange(B) if oracle_rows is None else np.asarray(sorted(oracle_rows))
    assert len(set(rows.tolist())) == len(rows) and rows.min() >= 0 and rows.max() < B, rows
    orc.streaming(len(rows))
    fs = cfg.frame_size
    mism, lats = [], {}
    worst, executed = 0.0, 0
    with m.streaming(B):
        for f in range(F):
            mask = np.ones(B, bool)
            if use_masks and B > 1:
                mask = rng.random(B) > 0.3
                mask[0] = True
            if use_masks and f == F // 2 and B > 1:
                rmask = np.zeros(B, bool); rmask[B - 1] = True
                orc.reset_streaming(rmask[rows])
                m.reset_streaming(torch.from_numpy(rmask).to(device))
                mask[B - 1] = True
            if oracle_rows is not None and f in (0, F - 1):
                mask[rows] = True
            orc.set_exec_mask(mask[rows])
            m.set_exec_mask(torch.from_numpy(mask).to(device))
            xf = x[..., f * fs:(f + 1) * fs]
            lat = orc.encode_to_latent(xf if oracle_rows is None else xf[rows])
            co = orc.quantize(lat)
            ce = m.encode(torch.from_numpy(xf).to(device)).cpu().numpy()
            po = orc.decode(co)
            cd = ce.copy()                      # the decoder is fed the CHECKER's codes on the checked rows (its own elsewhere)
            cd[rows] = co
            pe = m.decode(torch.from_numpy(cd).to(device)).cpu().numpy()
            for i, b in enumerate(rows):
                if not mask[b]:
                    continue
                executed += 1
                if oracle_rows is None:
                    assert np.array_equal(ce[b], co[i]), f"codes differ frame {f} row {b}: {ce[b].ravel()} vs {co[i].ravel()}"
                for k, t in np.argwhere(ce[b] != co[i]):
                    mism.append((f, int(i), int(k), int(t), int(ce[b, k, t]), int(co[i, k, t])))
                    lats[f] = lat
                err = float(np.abs(pe[b] - po[i]).max()) / (PCM_ATOL + PCM_RTOL * float(np.abs(po[i]).max()))
                worst = max(worst, err)
                assert err <= 1.0, f"pcm differs frame {f} row {b}: {err:.2f} x the tolerance"
        kernels = {}
        for which in ("encode", "decode"):
            kernels[which] = {}
            for _, kern in m.launch_list(which):
                kernels[which][kern] = kernels[which].get(kern, 0) + 1
    if mism:
        audit_code_mismatches(orc, lats, mism, max_vectors=1)
    return {"batch": B, "frames": F, "rows_checked": [int(r) for r in rows], "rows_executed": executed,
            "decisions_differing": len(mism), "worst_pcm_over_tol": worst, "kernels": kernels}


def check_c2_recipe(model_factory, device, cfg, B=8, F=200, K=8, seed=0, p_exec=0.5, max_flips=2, oracle_rows=None):
    """SURVEY.md 8d's C2 recipe against the oracle: B streams of 0.1 * N(0, 1) PCM plus a sine row, F frames, a random exec
    mask per frame and ONE mid-run `reset_streaming(mask)`.  Row 0 always executes and row 1 executes nine frames in ten, so
    that at the full size (context 250, two positions per frame) their KV rings WRAP inside the run (frame 126 for row 0):
    the state the benchmark runs in and, before round 4, no full-size parity test reached (transformer.py:236-288).  Codes
    equal on executed rows (near-tie flips audited, at most `max_flips` vectors), PCM of the oracle's codes within 2e-5.
    oracle_rows: the engine runs all B streams, the (slow, numpy) checker only these rows of the batch - streams are independent
    (`test_batch_rows_are_independent_and_graph_equals_eager`), and the GPU suite has a time budget; default: every row."""
    sd = random_mimi_state_dict(cfg, seed=1234)
    m = model_factory(sd, cfg, K)
    orc = MimiOracle(sd, cfg, num_codebooks=K)
    rng = np.random.default_rng(seed)
    fs = cfg.frame_size
    x = (0.1 * rng.standard_normal((B, 1, fs * F))).astype(np.float32)
    tt = np.arange(fs * F, dtype=np.float64) / cfg.sample_rate
    x[B - 1, 0] = (0.5 * np.sin(2 * np.pi * 440.0 * tt)).astype(np.float32)           # the C1 / C2 sine row
    pr = np.full(B, p_exec)
    pr[0] = 1.0
    if B > 1:
        pr[1] = 0.9
    reset_at = F // 2
    rmask = np.zeros(B, bool)
    rmask[B - 1] = True
    if B > 3:
        rmask[2] = True
    rows = np.arange(B) if oracle_rows is None else np.asarray(sorted(oracle_rows))
    executed = np.zeros(B, int)
    wrapped = False
    mism, lats = [], {}
    worst = 0.0
    orc.streaming(len(rows))
    with m.streaming(B):
        for f in range(F):
            if f == reset_at:
                orc.reset_streaming(rmask[rows])
                m.reset_streaming(torch.from_numpy(rmask).to(device))
                executed[rmask] = 0
            mask = rng.random(B) < pr
            orc.set_exec_mask(mask[rows])
            m.set_exec_mask(torch.from_numpy(mask).to(device))
            xf = x[..., f * fs:(f + 1) * fs]
            lat = orc.encode_to_latent(xf[rows])
            co = orc.quantize(lat)
            ce = m.encode(torch.from_numpy(xf).to(device)).cpu().numpy()
            po = orc.decode(co)
            cd = ce.copy()                      # the decoder is fed the CHECKER's codes on the checked rows (its own elsewhere)
            cd[rows] = co
            pe = m.decode(torch.from_numpy(cd).to(device)).cpu().numpy()
            executed += mask
            wrapped |= bool((executed[rows] * (fs // cfg.hop_length) > cfg.tr_context).any())
            for i, b in enumerate(rows):
                if not mask[b]:
                    continue
                for k, t in np.argwhere(ce[b] != co[i]):
                    mism.append((f, int(i), int(k), int(t), int(ce[b, k, t]), int(co[i, k, t])))
                    lats[f] = lat
                err = float(np.abs(pe[b] - po[i]).max()) / (PCM_ATOL + PCM_RTOL * float(np.abs(po[i]).max()))
                worst = max(worst, err)
                assert err <= 1.0, f"pcm differs frame {f} row {b}: {err:.2f} x the tolerance"
    total = int(executed.sum()) * K            # (an underestimate after the reset: the reset rows' earlier frames counted too)
    print(f"[parity] mimi C2 recipe B={B} F={F}: {len(mism)} index decisions differ on executed rows; worst PCM error "
          f"{worst:.3f} x tolerance; ring wrapped: {wrapped}")
    if mism:
        audit_code_mismatches(orc, lats, mism, max_vectors=max_flips)
    return {"frames": F, "batch": B, "rows_checked": [int(r) for r in rows], "decisions_differing": len(mism), "worst_pcm_over_tol": worst,
            "wrapped": wrapped}
