"""What the sub-commands share above the engine: engine_scope (who closes the context),
refusal / refuse_multi_rank, columns_in_header and read_labels (the checks before any GPU call), device_call / tested_rows (the device
round trip of a per-row test), write_event_table, and the readers of the PS table, the manifests and the GTF."""
import contextlib
import sys

import numpy as np


@contextlib.contextmanager
def engine_scope(ctx, make):
    """`with engine_scope(ctx, lambda: Context(device)) as ctx:` -> the caller's context, left open; without one the
    context make() returns, closed when the block ends, however it ends"""
    if ctx is not None:
        yield ctx
        return
    ctx = make()
    try:
        yield ctx
    finally:
        ctx.close()


def refusal(prefix):
    """-> refuse(why): prints `<prefix>: <why>. Exit.` to stderr and exits with status 1"""
    def refuse(why):
        print(f"{prefix}: {why}. Exit.", file=sys.stderr)
        sys.exit(1)
    return refuse


def refuse_multi_rank(L, message):
    """a command that runs in one process only: under the multi-rank launcher print its message and exit with status 1"""
    if L.world > 1:
        print(message, file=sys.stderr)
        sys.exit(1)


def columns_in_header(names, header_names, refuse):
    """-> int32 column index of every name, in the order of `names`; refuse()s a name that is not exactly once in the
    table header"""
    where = {}
    for j, name in enumerate(header_names):
        where.setdefault(name, []).append(j)
    for name in names:
        hits = where.get(name, [])
        if len(hits) != 1:
            refuse(f"sample {name!r} " + ("is missing from the table header" if not hits else
                                          f"appears {len(hits)} times in the table header"))
    return np.array([where[x][0] for x in names], dtype=np.int32)


def device_call(ctx, inputs, outputs, launch):
    """One device round trip.  inputs: name -> (host array, dtype), uploaded in order; outputs: name -> (shape, dtype)
    (engine.field_shapes), allocated in order; launch(d_in, d_out) queues the work on the two dicts of device arrays.
    -> name -> host copy of every output.  Every device array is freed, also when a step raises."""
    from . import _stages
    d_in, d_out = {}, {}
    try:
        with _stages.stage("h2d"):
            for name, (host, dtype) in inputs.items():
                d_in[name] = ctx.to_device(host, dtype)
            for name, (shape, dtype) in outputs.items():
                d_out[name] = ctx.empty(shape, dtype)
        with _stages.stage("kernels"):
            launch(d_in, d_out)
            ctx.sync()
        with _stages.stage("d2h"):
            return {name: a.to_host() for name, a in d_out.items()}
    finally:
        for a in (*d_in.values(), *d_out.values()):
            a.free()


def tested_rows(ctx, inputs, outputs, launch):
    """device_call for a per-row test whose outputs hold `tested` and `p`, with Benjamini-Hochberg over the tested rows on
    the resident vectors -> (keep: the indices of the tested rows, name -> the other outputs at those rows ([n] fields
    [keep], [k, n] fields [:, keep]) and `corrected`)"""
    n = outputs["p"][0]

    def test_and_correct(d_in, d_out):
        launch(d_in, d_out)
        ctx.bh_masked_dev(d_out["p"], d_out["tested"], d_out["corrected"])

    # (the corrected vector rides as `corrected`, what it is called in the result: no test's field has that name --
    # Friedman's Q is the field `q`)
    assert "corrected" not in outputs
    res = device_call(ctx, inputs, {**outputs, "corrected": (n, np.float64)}, test_and_correct)
    q = res.pop("corrected")
    keep = np.flatnonzero(res.pop("tested"))
    r = {name: v[keep] if v.ndim == 1 else np.ascontiguousarray(v[:, keep]) for name, v in res.items()}
    r["corrected"] = q[keep]
    return keep, r


def samples_from_manifest(path):
    """First whitespace-separated token of every line (compareSampleSets.py:105-115)."""
    with open(path) as fin:
        return [line.split()[0] for line in fin]


def read_labels(path, refuse):
    """a label file, one `sample<TAB>label` per line (labels are arbitrary strings; blank lines are skipped) -> sample ->
    the list of its labels in file order, so that the caller can tell a sample without a label from one with two;
    refuse()s a line without a tab"""
    labels = {}
    with open(path) as fin:
        for at, line in enumerate(fin, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            sample, tab, label = line.partition("\t")
            if not tab:
                refuse(f"line {at} of {path} is not `sample<TAB>label`")
            labels.setdefault(sample, []).append(label)
    return labels


def table_header_names(path):
    """the sample names of an `_allPS.tsv` header (its first line alone is read)"""
    with open(path) as fin:
        return fin.readline().strip().split("\t")[1:]


def read_ps_table(path, as_table=False):
    """`_allPS.tsv` -> (row names array, column names array, float32 matrix), :193-204.  as_table: the row names as a
    textio.NameTable (one byte string + offsets: a million-row table costs no Python string per row)."""
    from . import textio
    header, rows, matrix = textio.read_table_numeric(path, np.float32, as_table=as_table)     # text -> float64 -> float32, as numpy
    headers = header.strip().split("\t")[1:]
    return (rows if as_table else np.array(rows)), np.array(headers), matrix


def read_annotation(gtf_path):
    """GTF -> (junction -> gene names, (chrom,strand) -> {(start,stop): gene names},
    junction -> transcript ids); restates getAnnotated (compareSampleSets.py:32-93)."""
    def attr(info, key):
        return [x[1] for x in info if key in x[0]][0]

    gene_coords, genes, transcripts = {}, {}, {}
    with open(gtf_path) as gtf:
        for line in gtf:
            if line.startswith("#"):
                continue
            row = line.rstrip().split("\t")
            info = [x.split('"') for x in row[8].split(";")]
            chrom, strand = row[0], row[6]
            start, stop = int(row[3]), int(row[4]) - 1
            if row[2] == "transcript":
                tid = attr(info, "transcript_id")
                genes[tid] = attr(info, "gene_name")
                transcripts[(tid, chrom, strand)] = []
            elif row[2] == "exon":
                transcripts[(attr(info, "transcript_id"), chrom, strand)].append((start, stop))
            elif row[2] == "gene":
                gene_name = attr(info, "gene_name")
                attr(info, "gene_id")      # the reference requires the attribute to exist
                gene_coords.setdefault((chrom, strand), {}).setdefault((start, stop), []).append(gene_name)
    annotated, transcript_ids = {}, {}
    for (tid, chromosome, strand), exons in transcripts.items():
        for i in range(len(exons) - 1):
            junction = (chromosome, exons[i][1], exons[i + 1][0], strand)
            if junction in annotated:
                if genes[tid] not in annotated[junction]:
                    annotated[junction].append(genes[tid])
                    transcript_ids[junction].append(tid)
            else:
                annotated[junction] = [genes[tid]]
                transcript_ids[junction] = [tid]
    return annotated, gene_coords, transcript_ids


def annotation_suffixes(names, gtf_path):
    """'\\tgene\\toverlapping\\ttranscript_id' for every event name (compareSampleSets.py:238-264).  The reference
    walks all gene intervals of the event's (chromosome, strand) per event in Python; here that scan is the
    library's threaded interval join (sdice_interval_overlaps) and the known-junction look-ups stay dict
    look-ups; order of the listed genes = the reference's (dict order of the intervals, file order inside)."""
    from . import textio
    annotated, gene_coords, transcript_ids = read_annotation(gtf_path)
    groups = {key: g for g, key in enumerate(gene_coords)}
    grp_ptr = np.zeros(len(groups) + 1, dtype=np.int64)
    lo, hi, key_names = [], [], []
    for g, intervals in enumerate(gene_coords.values()):
        for (gene_start, gene_stop), gene_names in intervals.items():
            lo.append(gene_start)
            hi.append(gene_stop)
            key_names.append(",".join(gene_names))
        grp_ptr[g + 1] = len(lo)
    ev_group = np.empty(len(names), dtype=np.int32)
    ev_a = np.empty(len(names), dtype=np.int64)
    ev_b = np.empty(len(names), dtype=np.int64)
    junctions = []
    for n, name in enumerate(names):
        chromosome, coords, strand = name.split(":")
        start, stop = (int(x) for x in coords.split("-"))
        start -= 1
        stop += 1
        junctions.append((chromosome, start, stop, strand))
        ev_group[n] = groups.get((chromosome, strand), -1)
        ev_a[n] = start
        ev_b[n] = stop
    ptr, idx = textio.interval_overlaps(ev_group, ev_a, ev_b, grp_ptr, lo, hi)
    ptr = ptr.tolist()
    idx = idx.tolist()
    nan = ["nan"]
    return ["\t" + ",".join(annotated.get(j, nan)) + "\t" + ",".join(key_names[k] for k in idx[ptr[n]:ptr[n + 1]]) +
            "\t" + ",".join(transcript_ids.get(j, nan)) for n, j in enumerate(junctions)]


def write_event_table(path, header, rows, keep, columns, modes, annotation):
    """the kept events, one line each: name, the columns and, with a GTF, its gene / overlapping / transcript_id cells"""
    from . import _stages, textio
    names, suffixes = rows.take(keep), None
    if annotation:
        names = list(names)
        suffixes = annotation_suffixes(names, annotation)
        header += "\tgene\toverlapping\ttranscript_id"
    with _stages.stage("format+write"):
        textio.write_columns(path, header + "\n", names, columns, modes, suffixes=suffixes)
