"""Runs oracle/_ref/hts_witness: the reference's own htslib-1.3 behind a small program of this project
(oracle/hts_witness.c, built by `make -C oracle` where the reference tree exists).

The program and the library travel with the working tree but never enter git.  Where the program is missing although the
reference tree is there, that is a broken build and the caller fails with the command that mends it; a test is skipped
only where neither the program nor the reference tree exists, since nothing could then build it.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "oracle", "_ref", "hts_witness")


def _reference_tree():
    """Where oracle/Makefile looks for the reference: $REFERENCE, else the default its `REFERENCE ?=` line names."""
    m = re.search(r"^REFERENCE \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return os.environ.get("REFERENCE") or m.group(1)


REFERENCE = _reference_tree()


def available():
    """True where the program is there; False where neither it nor the reference tree is; fails where only the tree is."""
    if os.path.exists(PROGRAM):
        return True
    if os.path.exists(os.path.join(REFERENCE, "deps", "htslib-1.3", "sam.c")):
        pytest.fail(f"{PROGRAM} is missing although the reference tree is at {REFERENCE}: "
                    f"run `make -C {os.path.join(ROOT, 'oracle')} REFERENCE={REFERENCE}`", pytrace=False)
    return False


def program():
    if not available():
        pytest.skip(f"no {PROGRAM} and no reference tree at {REFERENCE} to build it from")
    return PROGRAM


def run(*args, stdin=None, ok=(0,)):
    """stdout of `hts_witness ARGS` as text; the exit status must be one of `ok`."""
    p = subprocess.run([program(), *[str(a) for a in args]], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode in ok, (args, p.returncode, p.stderr[-2000:])
    return p.stdout


def status(*args):
    return subprocess.run([program(), *[str(a) for a in args]], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode


# ---- the subcommands, parsed ------------------------------------------------------------------------------------------
def depth(bam):
    """[(tid, pos, depth)] of every position the pileup reports."""
    return [tuple(int(x) for x in line.split()) for line in run("depth", bam).splitlines()]


def records(bam):
    """(refs [(name, len)], records as dicts shaped like util_bam.read_bam's, plus 'end' and with cigar / seq as strings)."""
    lines = run("records", bam).split("\n")
    n_ref = int(lines[0].split()[1])
    refs = []
    for line in lines[1:1 + n_ref]:
        _, name, ln = line.split(" ")
        refs.append((name, int(ln)))
    recs = []
    for line in lines[1 + n_ref:]:
        if not line:
            continue
        tid, pos, end, flag, mapq, l_qseq, mtid, mpos, cigar, seq, name, xs = line.split("\t")
        if xs == "-":
            xs = None
        else:
            ty, val = xs.split(":")
            xs = (ty, chr(int(val)))
        recs.append(dict(tid=int(tid), pos=int(pos), end=int(end), flag=int(flag), mapq=int(mapq), l_qseq=int(l_qseq), mtid=int(mtid),
                         mpos=int(mpos), cigar=cigar, seq=seq, name=name, xs=xs))
    return refs, recs


def index(bam, out):
    run("index", bam, out)
    return open(out, "rb").read()


def query(bam, idx, regions):
    """[((tid, beg, end), [(pos, end, qname)])] for regions [(tid, beg, end)]: the records in the order htslib returns them."""
    text = run("query", bam, idx, stdin="".join(f"{t} {b} {e}\n" for t, b, e in regions))
    out, cur = [], None
    for line in text.splitlines():
        if line.startswith("#"):
            cur = []
            out.append((tuple(int(x) for x in line.split()[1:]), cur))
        elif line.startswith("!"):
            cur.append(line)
        else:
            pos, end, name = line.split(" ", 2)
            cur.append((int(pos), int(end), name))
    assert [k for k, _ in out] == [tuple(r) for r in regions]
    return out


def faidx(fa):
    """The exit status of fai_build (0 built FA.fai, 1 refused)."""
    return status("faidx", fa)


def fetch(fa, queries):
    """[(len, string)] of faidx_fetch_seq for queries [(name, beg, end)]."""
    text = run("fetch", fa, stdin="".join(f"{n} {b} {e}\n" for n, b, e in queries))
    out = []
    for line in text.split("\n")[:-1]:
        ln, _, s = line.partition(" ")
        out.append((int(ln), s))
    assert len(out) == len(queries)
    return out


def eof(path):
    return int(run("eof", path))
