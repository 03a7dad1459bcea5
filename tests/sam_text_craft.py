"""Crafted SAM texts for tests/test_sam_parse.py: each is there for one property, which the tests assert from the text
alone with Python's own bytes.find, bytes.split, re.findall and int.  Nothing here imports the code under test."""
import re

RUN = re.compile(b"[0-9]+[MIDNSHP=X]")


def rec(qname="q1", flag="0", rname="c1", pos="7", cigar="3M", seq="ACG", extra=(), end="\n"):
    return ("\t".join([qname, flag, rname, pos, "60", cigar, "*", "0", "0", seq, "*"] + list(extra)) + end).encode()


INT_FORMS = ["+4", "-1", "007", "4x", "1_0", "2147483648", "-2147483649", "2147483647", "-2147483648", "+", "-", "0"]
CIGAR_FORMS = ["*", "5MM", "12AB3M", "0012M", "3m", "4294967295M", "4294967296M", "7N2P1=1X", "5H4H3S10M2I", "10M3S5H", "1M1I" * 150,
               "1M" * 32, "1M" * 33, "2H3S" + "1M1I" * 40 + "4S5H", "99999999999999999999999M2M", "M", "3", "=5"]

TEXTS = {
    "empty": b"",
    "headers_only": b"@HD\tVN:1.6\n@SQ\tSN:c1\tLN:5\n@PG\tID:x\ta\tb\n@RG\tID:r\ta\tb\n@CO\ttext\there\tmore\n",
    "no_final_newline": rec() + rec(qname="q2")[:-1],
    "final_blank_line": rec() + b"\n",
    "crlf": rec(end="\r\n") + rec(qname="q2", end="\r\n"),
    "short_lines": rec() + b"x\n" + b"@P\n" + b"\n" + rec(qname="q2"),
    "header_prefix": b"@PGx\ta\tb\tc\td\n" + b"@XX\ta\tb\tc\n" + b"@pg\ta\tb\tc\n",
    "tabs_0": b"q 0 c1 1 60 3M * 0 0 ACG *\n" + b"q\n",
    "tabs_1": b"q\t0 c1 1 60 3M * 0 0 ACG *\n" + b"q\tr\n",
    "tabs_2": b"q\t0\tc1 1 60 3M * 0 0 ACG *\n" + b"q\tr\ts\n",
    "tabs_3": b"q\t0\tc1\t1 60 3M * 0 0 ACG *\n" + b"q\tr\tc1\tt\n",
    "ten_tokens_mid_chunk": b"".join(rec(qname="a%d" % i) for i in range(3)) + b"short\t0\tc1\t5\t60\t10M\t*\t0\t0\tACGT\n" +
                            b"".join(rec(qname="b%d" % i) for i in range(3)),
    "empty_tab_rname": b"q\t0\t\t1\t60\t3M\t*\t0\t0\tACG\t*\tNM:i:0\tAS:i:1\n",
    "space_in_field": b"q\t0\tc 1\t1\t60\t3M\t*\t0\t0\tACG\t*\n",
    "vt_ff": b"q\x0b0\x0cc1\t1\t60\t3M\t*\t0\t0\tACG\t*\n",
    "exactly_11": rec(),
    "more_than_11": rec(extra=("NM:i:1", "XX:Z:more")),
    "flag_forms": b"".join(rec(qname="f%d" % i, flag=v) for i, v in enumerate(INT_FORMS)),
    "pos_forms": b"".join(rec(qname="p%d" % i, pos=v) for i, v in enumerate(INT_FORMS)),
    "seq_star": rec(seq="*") + rec(qname="q2"),
    "cigar_forms": b"".join(rec(qname="g%d" % i, cigar=v) for i, v in enumerate(CIGAR_FORMS)),
    "chunks": rec(rname="c1") + b"@CO\tx\n" + b"junk\n" + rec(qname="q2", rname="c1") + rec(qname="q3", rname="c2") +
              rec(qname="q4", rname="c3") + b"\n" + rec(qname="q5", rname="c3") + rec(qname="q6", rname="c33") + rec(qname="q7", rname="c3"),
}

BOUNDARY = 256
BOUNDARY_RECORD = b"read_1\t16\tctg_9\t1234\t60\t120M5I77M\t*\t0\t0\tACGTACGT\t*\n"


def boundary_texts():
    """the same record behind a comment line of every length that lets one of its bytes be byte 256 of the text, and two
    more records after it"""
    out = []
    for start in range(BOUNDARY - len(BOUNDARY_RECORD) - 1, BOUNDARY + 3):
        head = b"@CO\t" + b"x" * (start - 5) + b"\n"
        assert len(head) == start
        out.append(head + BOUNDARY_RECORD + rec(rname="ctg_9") + rec(rname="other"))
    return out


def features(text):
    """positions in BOUNDARY_RECORD's copy inside text: line start, token starts, token ends (last byte), third tab, the
    digit runs of the CIGAR as (first, op byte)"""
    at = text.index(BOUNDARY_RECORD)
    line = BOUNDARY_RECORD
    starts, ends, k = [], [], 0
    for tok in line.split():
        k = line.index(tok, k)
        starts.append(at + k)
        ends.append(at + k + len(tok) - 1)
        k += len(tok)
    tabs = [at + i for i, b in enumerate(line) if b == 9]
    cigar_at = starts[5]
    runs = [(cigar_at + m.start(), cigar_at + m.end() - 1) for m in RUN.finditer(line.split()[5])]
    return dict(line_start=at, token_starts=starts, token_ends=ends, third_tab=tabs[2], runs=runs)
