"""tests/golden/top_p.json: the nucleus sizes of the reference's own `sample_token(x, True, temp, 0, p)` on the fixture rows of
tests/nucleus_cases.py (every row family at the four vocabularies with the p list, and the dyadic rows).

    python tests/golden/make_golden_top_p.py --ref <reference checkout>/moshi

The reference's utils/sampling.py is loaded by path, its `multinomial` is replaced with a recorder, and for each row the count of
non-zero entries of the `probs_sort` that `sample_top_p` hands to it is recorded.  The fixture is small: per row the kind and
family name, V, the seed, temp, p, that count and a CRC of the row's bytes - the rows themselves are regenerated from their seeds.
Nothing at test time imports the reference.
"""
import argparse
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's python package root (the directory that holds moshi/utils/sampling.py)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_sampling", Path(args.ref) / "moshi" / "utils" / "sampling.py")
    sampling = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sampling)
    from tests import nucleus_cases as nc

    seen = []

    def recorder(probs, num_samples=1, **kw):
        seen.append(int(torch.count_nonzero(probs)))
        return torch.zeros(*probs.shape[:-1], 1, dtype=torch.long)
    sampling.multinomial = recorder
    rows, worst = [], 0.0
    for kind, name, V, seed, temp, p, x in nc.fixture_rows():
        seen.clear()
        sampling.sample_token(torch.from_numpy(x), True, temp, 0, p)
        assert len(seen) == 1
        n_lo, n_hi = nc.nucleus_sizes(x, temp, p)
        if not n_lo <= seen[0] <= n_hi:
            print(f"outside the bracket: {kind} {name} V={V} seed={seed} temp={temp} p={p}: reference {seen[0]}, bracket [{n_lo}, {n_hi}]")
            worst = max(worst, 1.0)
        rows.append([kind, name, V, seed, temp, p, seen[0], nc.crc(x)])
    out = HERE / "top_p.json"
    out.write_text(json.dumps({"delta": nc.DELTA, "columns": ["kind", "name", "V", "seed", "temp", "p", "reference_nucleus_size", "crc32"],
                               "rows": rows}, separators=(",", ":")).replace("],[", "],\n["))
    print(f"{out}: {len(rows)} rows, {out.stat().st_size} bytes; rows outside the bracket: {int(worst)}")


if __name__ == "__main__":
    main()
