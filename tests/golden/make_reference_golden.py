#!/usr/bin/env python3
"""Record what the REFERENCE's own BSDF code computes, as data: tests/golden/reference_bsdf.npz.

Runs oracle/_ref/libptref_om.so (the reference's headers host-compiled by oracle/Makefile behind
oracle/ptref_capi.cpp, with the oracle's sin/cos/exp polynomials behind sinf/cosf/expf) over a
deterministic subset of the input set of tests/test_oracle_vs_reference.py: every edge case and
every GOLDEN_STRIDE-th random case of each (model, roughness).  The file holds results only, as
integer bit patterns; the inputs are rebuilt from their seeds by the test, which asserts that the
oracle reproduces these bits where the reference tree does not exist.

    python tests/golden/make_reference_golden.py     # needs oracle/_ref/ (make -C oracle)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_oracle_vs_reference as T  # noqa: E402

OUT = Path(__file__).resolve().parent / "reference_bsdf.npz"


def make(lib) -> dict:
    ref = T.reference_side(lib)
    rows = {k: [] for k in ("sample_ok", "sample_out", "sample_seed", "eval_f", "eval_seed", "pdf")}
    offset = [0]
    for model, ri in T.PAIRS:
        full = T.build_cases(model, ri)
        c = T.subset(full, T.golden_index(full))
        ok, out, seed = T.run_sample(ref, c)
        f, fs, p = T.run_eval_pdf(ref, T.with_sampled(c, out))
        rows["sample_ok"].append(ok.astype(np.uint8))
        rows["sample_out"].append(out)
        rows["sample_seed"].append(seed)
        rows["eval_f"].append(f)
        rows["eval_seed"].append(fs)
        rows["pdf"].append(p)
        offset.append(offset[-1] + len(ok))
    g = {k: np.concatenate(v) for k, v in rows.items()}
    g["offset"] = np.array(offset, dtype=np.int64)
    return g


if __name__ == "__main__":
    if not T.REF_OM.exists():
        sys.exit(f"{T.REF_OM} is missing: build it with `make -C oracle` where the reference tree exists")
    np.savez_compressed(OUT, **make(T.load_reference(T.REF_OM)))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
