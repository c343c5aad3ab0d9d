#!/usr/bin/env python3
"""Measures the oracle's shading layer against the float64 restatement (tests/shading_reference.py) over the families of tests/shading_cases.py and
writes tests/golden/shading_layer.json: per function the worst error over the random `bulk` families, in units of max(ulp32(|value|),
ulp32(1) * scale), and the bound tests/test_shading_cases.py asserts on every family — twice that, because the bulk set is a sample.  CPU only.

    python tools/shading_bounds.py            # print the table, compare with the stored file
    python tools/shading_bounds.py --write    # store it

CLASS_ONLY below is reasoning, not measurement: the families on which a function's error against float64 has no bound, and why."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import shading_cases as sc          # noqa: E402
import shading_reference as sr      # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "shading_layer.json")
CLASS_ONLY = {
    "sample_texture": dict(families=["beyond_int_range_1x1", "beyond_int_range_2x3", "beyond_int_range_5x7", "beyond_int_range_8x8"],
                           reason="|u * w| >= 2^31: fp32 holds no fraction there (both weights are 1 and 0) where float64 still has one, and the texel index is the "
                                  "saturated one by decree, not the mathematical wrap"),
}


def measure(oracle):
    worst, per_family = {}, {}
    for mode in range(12):
        for c in sc.cases(mode):
            out = oracle.selftest_shading(mode, c.inp, c.tables, c.nout)
            for chk in sr.reference(c):
                if chk.discrete or set(chk.planes) & set(c.expect):
                    continue
                e = sr.error_units(out, chk)
                w = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
                per_family[(chk.function, c.family)] = max(per_family.get((chk.function, c.family), 0.0), w)
                if c.family == "bulk":
                    worst[chk.function] = max(worst.get(chk.function, 0.0), w)
    return worst, per_family


def main():
    from oracle import pyoracle as po
    po.build()
    worst, per_family = measure(po)
    doc = dict(unit="error of the oracle against float64 in units of max(ulp32(|float64 value|), ulp32(1) * scale); scale: tests/shading_reference.py",
               rule="bound = 2 * the worst error over the bulk families (a sample; the oracle is what is measured, not the device)",
               functions={f: dict(bulk_worst=float(f"{w:.6g}"), bound=float(f"{2 * w:.6g}")) for f, w in sorted(worst.items())}, class_only=CLASS_ONLY)
    for (f, fam), w in sorted(per_family.items()):
        over = w > 2 * worst[f] and fam not in CLASS_ONLY.get(f, {}).get("families", [])
        print(f"{f:36s} {fam:30s} {w:12.4g}  (bulk {worst[f]:.4g}){'   OVER THE BOUND' if over else ''}")
    if "--write" in sys.argv:
        with open(PATH, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", PATH)
    elif os.path.exists(PATH):
        print("stored file", "matches" if json.load(open(PATH))["functions"] == doc["functions"] else "DIFFERS")


if __name__ == "__main__":
    main()
