"""GPU: a sub-command that is handed no engine makes one, runs on it and closes it -- the path of the command line, which
every other GPU test bypasses by passing the session context.  The files of both runs must be the same bytes.

Input: the 300 x 12 golden compare table (tests/golden/compare) and its two manifests.
"""
import argparse
import os

import pytest

pytestmark = pytest.mark.gpu


def _inputs(golden_dir, tmp_path):
    d = os.path.join(golden_dir, "compare")
    table = os.path.join(d, "in_allPS.tsv")
    header = open(table).readline().rstrip("\n").split("\t")[1:]
    lines1, lines2 = open(os.path.join(d, "m1.tsv")).readlines(), open(os.path.join(d, "m2.tsv")).readlines()
    assert len(header) == 12 and len(lines1) == 7 and len(lines2) == 6
    files = {"pair1": "".join(lines1[:6]),                                   # (equal length: the seventh names no column)
             "first3": "".join(lines1[:3]), "third": "".join(f"{x}\n" for x in header[3:6]),
             "covariate": "".join(f"{x}\t{j}\n" for j, x in enumerate(header))}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    return table, os.path.join(d, "m1.tsv"), os.path.join(d, "m2.tsv"), {k: str(tmp_path / k) for k in files}


def _commands(golden_dir, tmp_path):
    """-> [(name, run_with, the namespace without its output, the output attribute, the suffixes of the files written)]"""
    from splicedice_amd import compare_sample_sets as css, correlate, sample_matrix
    table, m1, m2, made = _inputs(golden_dir, tmp_path)
    two = dict(psiSPLICEDICE=table, manifest2=m2, annotation="")
    return [
        ("two_sets", css.run_with, dict(two, manifest1=m1), "outputFile", [""]),
        ("paired", css.run_with, dict(two, manifest1=made["pair1"], paired=True), "outputFile", [""]),
        ("three_sets", css.run_with, dict(two, manifest1=made["first3"], moreManifests=[made["third"]]), "outputFile", [""]),
        ("correlate", correlate.run_with, dict(psiSPLICEDICE=table, covariate=made["covariate"], annotation=""), "outputFile", [""]),
        ("sample_matrix", sample_matrix.run_with, dict(psiSPLICEDICE=table, samples="", minShared=3), "outputPrefix",
         ["_sampleCorrelation.tsv", "_sampleDistance.tsv", "_sampleShared.tsv"]),
    ]


@pytest.mark.parametrize("name", ["two_sets", "paired", "three_sets", "correlate", "sample_matrix"])
def test_a_command_on_its_own_context_writes_the_bytes_of_the_shared_one(ctx, golden_dir, tmp_path, name):
    _, run_with, fields, out_attr, suffixes = next(c for c in _commands(golden_dir, tmp_path) if c[0] == name)
    outs = {}
    for who, engine in (("shared", ctx), ("own", None)):
        prefix = str(tmp_path / f"{name}_{who}")
        run_with(argparse.Namespace(**fields, **{out_attr: prefix}), ctx=engine)
        outs[who] = [open(prefix + sfx, "rb").read() for sfx in suffixes]
    assert outs["shared"] == outs["own"]
    assert all(len(data.splitlines()) > 10 for data in outs["own"])          # (a table, not a header alone)
    assert ctx.h                                                             # (the session context stays open)
