#!/usr/bin/env python3
"""Golden fixtures for the edge cases of `splicedice similarity` and `splicedice findOutliers` by RUNNING THE REFERENCE
modules on the hand-made inputs of tests/scoring_fixtures.py.

Build-container only (it needs the reference checkout).  Writes

  tests/golden/similarity_edge/   in_vs.tsv, in_allPS.tsv, in_allPS_nan_column.tsv, the two manifests and per case
                                  expected_<case>.tsv (what the reference wrote, all of it or the part before it raised)
                                  and expected_<case>.json (the inputs' file names and the exception's type name or null)
  tests/golden/outliers_edge/     matrix_f32.npz, matrix_f64.npz (120 x 24), samples.tsv, null.tsv and per matrix and
                                  cut-off expected_<f32|f64>_cutoff<0|2|3>.txt (the reference's stdout)

    python tests/golden/make_golden_scoring.py
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import pathlib
import shutil
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import scoring_fixtures as SF  # noqa: E402

OUTLIER_SHAPE = (120, 24)
CUTOFFS = (0, 2, 3)


def reference_module(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "splicedice", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def fresh(name):
    out = pathlib.Path(HERE) / name
    shutil.rmtree(out, ignore_errors=True)
    out.mkdir()
    return out


def similarity_edge():
    sim = reference_module("similarity")
    out = fresh("similarity_edge")
    for case in SF.SIMILARITY_CASES:
        vs, ps, manifest = SF.write_similarity_case(out, case)
        report, raised = out / f"expected_{case}.tsv", None
        try:
            sim.run_with(argparse.Namespace(comparison=vs, allps=ps, manifest=manifest, output=str(report)))
        except Exception as e:                      # noqa: BLE001 (the point is to record what the reference raises)
            raised = type(e).__name__
        with open(out / f"expected_{case}.json", "w") as f:
            json.dump(dict(comparison=os.path.basename(vs), allps=os.path.basename(ps),
                           manifest=manifest and os.path.basename(manifest), raises=raised), f, indent=1)
            f.write("\n")
        print("similarity_edge", case, raised, len(report.read_text().splitlines()), "lines")


def outliers_edge():
    fo = reference_module("findOutliers")
    out = fresh("outliers_edge")
    for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
        t = SF.outlier_table(dtype, *OUTLIER_SHAPE)
        np.savez_compressed(out / f"matrix_{tag}.npz", cols=t["cols"], rows=t["rows"], data=t["data"])
        samples, null = SF.write_manifest(out / "samples.tsv", t["samples"]), SF.write_manifest(out / "null.tsv", t["null"])
        for cutoff in CUTOFFS:
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fo.run_with(argparse.Namespace(psiSPLICEDICE=str(out / f"matrix_{tag}.npz"), manifest=samples, nullMan=null,
                                               outlierCutoff=cutoff, dpsiThrsh=0.1))
            (out / f"expected_{tag}_cutoff{cutoff}.txt").write_text(buf.getvalue())
            print("outliers_edge", tag, cutoff, len(buf.getvalue().splitlines()), "lines")


if __name__ == "__main__":
    similarity_edge()
    outliers_edge()
