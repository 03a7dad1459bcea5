"""fg_sam_parse restated in plain Python, bytes to arrays: the contract of include/flye_gpu.h written with bytes.find,
bytes.split, re.findall and int, the very calls of the reference's SAM reader (flye/utils/sam_parser.py:168-213, :355-377,
:140).  It imports nothing of the code under test.  parse(text) returns a dict with the fields of struct fg_sam_text under
their names (numpy arrays of the header's types; the counts as int)."""
import re

import numpy as np

HEADERS = (b"@PG", b"@HD", b"@SQ", b"@RG", b"@CO")
RUN = re.compile(b"[0-9]+[MIDNSHP=X]")
INT = re.compile(b"[+-]?[0-9]+")
FIELDS = (("chunk_off", np.uint64), ("line_no", np.uint64), ("line_off", np.uint64), ("line_len", np.uint32), ("status", np.uint8),
          ("tab_rname_off", np.uint64), ("tab_rname_len", np.uint32), ("qname_off", np.uint64), ("qname_len", np.uint32),
          ("rname_off", np.uint64), ("rname_len", np.uint32), ("cigar_off", np.uint64), ("cigar_len", np.uint32),
          ("seq_off", np.uint64), ("seq_len", np.uint32), ("flag", np.int32), ("pos", np.int32), ("qry_start", np.int64),
          ("qry_end", np.int64), ("run_off", np.uint64), ("run_op", np.uint8), ("run_len", np.uint32))
COUNTS = ("n_lines", "n_records", "n_chunks", "n_runs")
TOKEN_NAMES = {0: "qname", 2: "rname", 5: "cigar", 9: "seq"}


def lines_of(text):
    """[(offset, line without its newline)]: split at 0x0A, a final 0x0A starts no further line"""
    out, at = [], 0
    while at < len(text):
        end = text.find(b"\n", at)
        if end < 0:
            end = len(text)
        out.append((at, text[at:end]))
        at = end + 1
    return out


def token_spans(line):
    """[(start, end)] of the tokens of line.strip().split(), found by searching each in turn"""
    spans, at = [], 0
    for tok in line.split():
        at = line.index(tok, at)
        spans.append((at, at + len(tok)))
        at += len(tok)
    return spans


def int32_of(tok):
    """(value, ok): ok when the token reads [+-]?[0-9]+ and fits int32"""
    if INT.fullmatch(tok) and -2 ** 31 <= int(tok) < 2 ** 31:
        return int(tok), True
    return 0, False


def span_of(runs):
    """(qry_start, qry_end) from [(op, len)]"""
    hard_left = runs[0][1] if runs and runs[0][0] == ord("H") else 0
    rest = [r for r in runs if r[0] != ord("H")]
    soft_left = rest[0][1] if rest and rest[0][0] == ord("S") else 0
    qry_pos = sum(n for op, n in runs if op in b"MIS")
    return hard_left + soft_left, qry_pos + hard_left - (sum(n for op, n in runs if op == ord("S")) - soft_left)


def parse(text):
    out = {k: [] for k, _ in FIELDS}
    out["chunk_off"], out["run_off"] = [], [0]
    last_name = None
    lines = lines_of(text)
    for no, (off, line) in enumerate(lines, 1):
        if line[:3] in HEADERS:
            continue
        tab_1 = line.find(b"\t")
        tab_2 = line.find(b"\t", tab_1 + 1) if tab_1 >= 0 else -1
        tab_3 = line.find(b"\t", tab_2 + 1) if tab_2 >= 0 else -1
        if tab_3 < 0:
            continue
        name = line[tab_2 + 1:tab_3]
        if name != last_name:
            out["chunk_off"].append(len(out["line_no"]))
            last_name = name
        out["line_no"].append(no); out["line_off"].append(off); out["line_len"].append(len(line))
        out["tab_rname_off"].append(off + tab_2 + 1); out["tab_rname_len"].append(len(name))
        spans = token_spans(line)
        status, flag, pos, runs = 0, 0, 0, []
        if len(spans) < 11:
            status = 1
            for k in TOKEN_NAMES.values():
                out[k + "_off"].append(0); out[k + "_len"].append(0)
        else:
            tok = [line[a:b] for a, b in spans]
            for i, k in TOKEN_NAMES.items():
                out[k + "_off"].append(off + spans[i][0]); out[k + "_len"].append(spans[i][1] - spans[i][0])
            flag, ok = int32_of(tok[1])
            status |= 0 if ok else 2
            pos, ok = int32_of(tok[3])
            status |= 0 if ok else 4
            status |= 8 if tok[9] == b"*" else 0
            for t in RUN.findall(tok[5]):
                n = int(t[:-1])
                if n >= 2 ** 32:
                    status |= 16
                    n = 0
                runs.append((t[-1], n))
        start, end = span_of(runs)
        out["status"].append(status); out["flag"].append(flag); out["pos"].append(pos)
        out["qry_start"].append(start); out["qry_end"].append(end)
        out["run_op"] += [op for op, _ in runs]; out["run_len"] += [n for _, n in runs]
        out["run_off"].append(len(out["run_op"]))
    out["chunk_off"].append(len(out["line_no"]))
    res = {k: np.array(out[k], dt) for k, dt in FIELDS}
    res.update(n_lines=len(lines), n_records=len(out["line_no"]), n_chunks=len(out["chunk_off"]) - 1, n_runs=len(out["run_op"]))
    return res


def token(text, res, r, which):
    """the bytes of a token of record r: which in qname, rname, cigar, seq, tab_rname, line"""
    a = int(res[which + "_off"][r])
    return text[a:a + int(res[which + "_len"][r])]
