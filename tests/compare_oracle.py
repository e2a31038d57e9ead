"""The comparison of an alignment E with a reference alignment R of the same rows (include/twl_compare.h), stated twice in plain Python:

  per_column(E, R)    per E column a dictionary from R column to the number of rows that put a residue into both
  brute_force(E, R)   every pair of rows, every pair of columns: O(n^2 W), for small inputs

Rows are bytes; only b'-' is a gap.  Both return the same dictionary of numpy arrays (shared uint64, letters, distinct uint32, recovered uint8,
all [We]; ref_letters uint32 [Wr]); agree() holds them to each other.  check_rows() is the rule of the refusal: (row, "count" | "letters") of the
smallest row that differs, or None.  report() is the line the command line prints."""
import numpy as np

GAP = 0x2D


def positions(row: bytes):
    """The columns of the row's letters, in order."""
    return [c for c, b in enumerate(row) if b != GAP]


def fold(b: int) -> int:
    return b - 32 if 0x61 <= b <= 0x7A else b


def check_rows(E, R):
    for k, (e, r) in enumerate(zip(E, R)):
        le = [fold(b) for b in e if b != GAP]
        lr = [fold(b) for b in r if b != GAP]
        if len(le) != len(lr):
            return k, "count"
        if le != lr:
            return k, "letters"
    return None


def _pack(We, Wr, shared, letters, distinct, recovered, ref_letters):
    return {"shared": np.array(shared, dtype=np.uint64).reshape(We), "letters": np.array(letters, dtype=np.uint32).reshape(We),
            "distinct": np.array(distinct, dtype=np.uint32).reshape(We), "recovered": np.array(recovered, dtype=np.uint8).reshape(We),
            "ref_letters": np.array(ref_letters, dtype=np.uint32).reshape(Wr)}


def per_column(E, R):
    assert check_rows(E, R) is None
    We, Wr = len(E[0]), len(R[0])
    cells = [dict() for _ in range(We)]
    nR = [0] * Wr
    for e, r in zip(E, R):
        for c, b in zip(positions(e), positions(r)):
            cells[c][b] = cells[c].get(b, 0) + 1
            nR[b] += 1
    shared = [sum(k * (k - 1) // 2 for k in d.values()) for d in cells]
    letters = [sum(d.values()) for d in cells]
    distinct = [len(d) for d in cells]
    recovered = [1 if len(d) == 1 and letters[c] >= 2 and nR[next(iter(d))] == letters[c] else 0 for c, d in enumerate(cells)]
    return _pack(We, Wr, shared, letters, distinct, recovered, nR)


def brute_force(E, R):
    """No keys: row pairs.  shared[c] = pairs of rows with residues in E column c that R puts into one column; a column is recovered when the
    set of its residues equals the set of residues of one R column and holds two or more."""
    assert check_rows(E, R) is None
    n, We, Wr = len(E), len(E[0]), len(R[0])
    pe = [positions(e) for e in E]
    pr = [positions(r) for r in R]
    colR = [dict(zip(pe[k], pr[k])) for k in range(n)]        # E column -> R column of row k's residue there
    shared = [0] * We
    for i in range(n):
        for j in range(i + 1, n):
            for c, b in colR[i].items():
                if colR[j].get(c) == b:
                    shared[c] += 1
    letters = [sum(1 for k in range(n) if c in colR[k]) for c in range(We)]
    distinct = [len({colR[k][c] for k in range(n) if c in colR[k]}) for c in range(We)]
    resE = [frozenset((k, pe[k].index(c)) for k in range(n) if c in colR[k]) for c in range(We)]
    resR = [frozenset((k, pr[k].index(b)) for k in range(n) if b in pr[k]) for b in range(Wr)]
    big = {s for s in resR if len(s) >= 2}
    recovered = [1 if s in big else 0 for s in resE]
    return _pack(We, Wr, shared, letters, distinct, recovered, [len(s) for s in resR])


def agree(E, R):
    a, b = per_column(E, R), brute_force(E, R)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    return a


def totals(cols):
    le = [int(x) for x in cols["letters"]]
    lr = [int(x) for x in cols["ref_letters"]]
    return {"shared": sum(int(x) for x in cols["shared"]), "pairs_out": sum(x * (x - 1) // 2 for x in le), "pairs_ref": sum(x * (x - 1) // 2 for x in lr),
            "recovered": int(cols["recovered"].sum()), "ref_columns": sum(1 for x in lr if x >= 2)}


def ratio(a: int, b: int) -> str:
    return "nan" if b == 0 else "%.6f" % (float(a) / float(b))


def report(cols, rows: int, only_out: int, only_ref: int) -> str:
    t = totals(cols)
    return (f"compare: rows {rows} ({only_out} only in the output, {only_ref} only in the reference) pairs_out {t['pairs_out']} pairs_ref {t['pairs_ref']} "
            f"shared {t['shared']} SP {ratio(t['shared'], t['pairs_ref'])} modeler {ratio(t['shared'], t['pairs_out'])} TC {t['recovered']}/{t['ref_columns']} "
            f"columns {len(cols['letters'])}/{len(cols['ref_letters'])}")


def header_lines(cols, rows: int, only_out: int, only_ref: int):
    """The "#key<TAB>value" lines --write-compare starts with: every number of the report line."""
    t = totals(cols)
    return [f"#rows\t{rows}", f"#only_in_output\t{only_out}", f"#only_in_reference\t{only_ref}", f"#pairs_out\t{t['pairs_out']}", f"#pairs_ref\t{t['pairs_ref']}",
            f"#shared\t{t['shared']}", f"#SP\t{ratio(t['shared'], t['pairs_ref'])}", f"#modeler\t{ratio(t['shared'], t['pairs_out'])}", f"#TC_recovered\t{t['recovered']}",
            f"#TC_columns\t{t['ref_columns']}", f"#columns_out\t{len(cols['letters'])}", f"#columns_ref\t{len(cols['ref_letters'])}"]


def column_lines(cols):
    """The per-column lines of --write-compare: column, letters, pairs, shared, distinct, recovered."""
    out = []
    for c in range(len(cols["letters"])):
        n = int(cols["letters"][c])
        out.append(f"{c}\t{n}\t{n * (n - 1) // 2}\t{int(cols['shared'][c])}\t{int(cols['distinct'][c])}\t{int(cols['recovered'][c])}")
    return out


def read_alignment(path, limit=None):
    """The reader's rule: name = first word, a duplicate keeps its first record, .gz accepted.  Returns (names, {name: row bytes}); with a limit,
    of the first `limit` distinct records only."""
    import gzip

    op = gzip.open if str(path).endswith(".gz") else open
    names, rows, cur = [], {}, None
    with op(path, "rb") as f:
        for line in f:
            line = line.strip()
            if line.startswith(b">"):
                w = line[1:].split()
                cur = w[0].decode() if w else ""
                if cur in rows:
                    cur = None
                elif limit is not None and len(names) == limit:
                    break
                else:
                    names.append(cur)
                    rows[cur] = b""
            elif cur is not None:
                rows[cur] += b"".join(line.split())
    return names, rows


def compare_files(est_path, ref_path):
    """What the command line computes on two files: (the report line, the lines of --write-compare)."""
    en, er = read_alignment(est_path)
    rn, rr = read_alignment(ref_path)
    common = [x for x in en if x in rr]
    cols = per_column_np([er[x] for x in common], [rr[x] for x in common])
    a, b = len(en) - len(common), len(rn) - len(common)
    return report(cols, len(common), a, b), header_lines(cols, len(common), a, b) + column_lines(cols)


def per_column_np(E, R):
    """per_column with numpy, for the larger seeded families: the residues of both alignments in row-major order are the same residues in the
    same order, so (E column, R column) of every residue is one zip of two nonzero() results; cells are counted by np.unique."""
    e = np.frombuffer(b"".join(E), dtype=np.uint8).reshape(len(E), -1) if len(E[0]) else np.zeros((len(E), 0), np.uint8)
    r = np.frombuffer(b"".join(R), dtype=np.uint8).reshape(len(R), -1) if len(R[0]) else np.zeros((len(R), 0), np.uint8)
    We, Wr = e.shape[1], r.shape[1]
    ke, c = np.nonzero(e != GAP)
    kr, b = np.nonzero(r != GAP)
    assert np.array_equal(ke, kr), "letter counts differ"
    cell, k = np.unique(c.astype(np.int64) * max(1, Wr) + b, return_counts=True)
    cc, bb = cell // max(1, Wr), cell % max(1, Wr)
    k = k.astype(np.uint64)
    shared = np.zeros(We, np.uint64)
    np.add.at(shared, cc, k * (k - np.uint64(1)) // np.uint64(2))
    letters = np.bincount(c, minlength=We).astype(np.uint32)
    nR = np.bincount(b, minlength=Wr).astype(np.uint32)
    distinct = np.bincount(cc, minlength=We).astype(np.uint32)
    recovered = np.zeros(We, np.uint8)
    single = distinct[cc] == 1
    recovered[cc[single]] = ((letters[cc[single]] >= 2) & (nR[bb[single]] == letters[cc[single]])).astype(np.uint8)
    return {"shared": shared, "letters": letters, "distinct": distinct, "recovered": recovered, "ref_letters": nR}
