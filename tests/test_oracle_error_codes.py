"""The catalogue of tests/error_cases.py against the CPU oracle: every entry raises exactly its code, the read number in the
message (BAD_XS, ANCHOR_MISMATCH, UNSORTED carry one) is the listed read, the clean background raises nothing, and every fault
planted into it raises its code at its ordinal.  Runs without a GPU and keeps the catalogue honest."""
import re

import numpy as np
import pytest

import error_cases as ec
from oracle import oracle as orc
from portcullis_amd.records import ReadBatch

READ_NUMBER = {-1: r"on read (\d+)", -7: r", read (\d+)", -14: r"sorted at (\d+)"}


def oracle_outcome(genome, reads, orientation="UNKNOWN", tid=0):
    """("ok", rows, region) or (code, message, read number in the message or None)."""
    try:
        rows, reg = orc.find_juncs(tid, len(genome), genome, ReadBatch.from_reads(reads), orientation)
    except orc.OracleError as e:
        m = re.search(READ_NUMBER[e.code], str(e)) if e.code in READ_NUMBER else None
        return e.code, str(e), (int(m.group(1)) if m else None)
    return "ok", rows, reg


def test_every_code_has_an_entry_or_a_reason():
    have = {f.code for f in ec.CATALOGUE}
    for code in list(range(-14, 0)) + [-20, -21]:
        assert (code in have) != (code in ec.NO_INPUT), code
    assert {-1, -2, -3, -4, -7, -10, -13, -14, -21} <= have
    for code, name in ec.NO_INPUT.items():
        assert re.search(rf"^ {code}\s+{name}\s", ec.__doc__, re.M), f"no written reason for {code}"


@pytest.mark.parametrize("name", [f.name for f in ec.CATALOGUE if f.oracle is not None])
@pytest.mark.parametrize("orientation", ["UNKNOWN", "FR"])
def test_oracle_raises_the_listed_code(name, orientation):
    f = ec.BY_NAME[name]
    assert [r["pos"] for r in f.reads] == sorted(r["pos"] for r in f.reads) or f.code == -14
    code, msg, read = oracle_outcome(ec.G, f.reads, orientation)
    assert code == f.oracle == f.code, (code, msg)
    if code in READ_NUMBER:
        assert read == f.at, msg
    if f.at != ec.WINDOW:  # the fault is that read's alone: the others give rows
        rest = [r for k, r in enumerate(f.reads) if k != f.at]
        assert oracle_outcome(ec.G, rest, orientation)[0] == "ok"


def test_device_only_entries_are_not_oracle_conditions():
    """NO_SEQ: the record is fine for the reference but for the bases nobody handed over -- with them the oracle gives rows."""
    for f in ec.CATALOGUE:
        if f.oracle is None:
            assert f.code == -21
            whole = [ec.rd(r["pos"], r["cigar"]) if r.get("l_qseq") else r for r in f.reads]
            assert oracle_outcome(ec.G, whole)[0] == "ok"


@pytest.fixture(scope="module")
def clean():
    return ec.background()


def test_background_is_clean(clean):
    genome, reads = clean
    assert len(reads) == ec.BACKGROUND_READS == 2 * 1024 + 300
    # the whole tiles -- of the one batch, and of batch two when the reads are cut at 1000 -- fit k1_count's whole-tile path, with
    # room for the few operations a planted fault adds (a background of long reads with indels takes the rounds path everywhere)
    whole = ReadBatch.from_reads(reads)
    ops = ec.whole_tile_ops(whole) + ec.whole_tile_ops(whole, 1000)
    assert len(ops) == 3 and max(ops) + 3 + 16 <= ec.K1C_OPSW, ops
    for ori in ("UNKNOWN", "FR"):
        out = oracle_outcome(genome, reads, ori)
        assert out[0] == "ok" and len(out[1]) > 10


@pytest.mark.parametrize("kind", sorted(ec.PLANTS))
def test_planted_faults(clean, kind):
    genome, reads = clean
    _, code, in_oracle, first = ec.PLANTS[kind]
    for k in ec.SWEEP_ORDINALS:
        if k < first:
            continue
        bad = ec.plant(genome, reads, kind, k)
        assert len(bad) == len(reads)
        unsorted = [i for i in range(1, len(bad)) if bad[i]["pos"] < bad[i - 1]["pos"]]
        assert unsorted == ([k] if kind == "UNSORTED" else [])
        if not in_oracle:
            continue
        got, msg, read = oracle_outcome(genome, bad, "FR")
        assert got == code, (k, msg)
        if code in READ_NUMBER:
            assert read == k, msg


def test_window_fault_behind_the_background(clean):
    genome, reads = clean
    got, msg, _ = oracle_outcome(genome, reads + [ec.window_fault_read(len(genome))], "FR")
    assert got == -10, msg


def test_two_phase_order_of_the_reference():
    """The reference walks all reads first and then junction by junction: with read 0 = 50M100N (NO_PRESENCE, found when its
    junction is processed) and read 1 carrying XS '*' (found in the read loop) it reports read 1's BAD_XS.  The device contract
    is the lowest ordinal instead (tests/test_gpu_error_parity.py)."""
    reads = [dict(pos=1000, cigar="50M100N", seq=ec.G[1000:1050], xs="+"), dict(pos=1010, cigar="50M", seq=None, xs="*")]
    code, msg, read = oracle_outcome(ec.G, reads)
    assert (code, read) == (-1, 1), msg


def test_fuzz_found_only_empty_anchors():
    """FUZZ_FOUND_ONLY_EMPTY_ANCHORS: the reason the catalogue gives for DIVERGENT (and for ANCHOR_MISMATCH being "0 vs 0" only) is an
    argument about the two walks; this looks for a counter-example among CIGARs of short operations of every kind (zero lengths,
    back and pad operations, clips in the middle), a second read widening the windows."""
    rng = np.random.default_rng(2024)
    seen = set()
    for _ in range(1500):
        ops = []
        for _k in range(int(rng.integers(2, 9))):
            ops.append((int(rng.choice([0, 1, 2, 3, 7])), str(rng.choice(list("MMMIDNNSHP=XB")))))
        at = int(rng.integers(0, len(ops) + 1))
        ops.insert(at, (int(rng.integers(1, 30)), "N"))
        cig = np.array([(l << 4) | "MIDNSHP=XB".index(o) for l, o in ops], np.uint32)
        lq = sum(l for l, o in ops if o in "MIS=X")
        pos = 1000 + int(rng.integers(0, 5))
        r = dict(pos=pos, cigar=cig, seq="".join(rng.choice(list("ACGT"), size=lq)) if lq else None, xs="+")
        wide = ec.rd(pos, "40M100N40M") if rng.random() < 0.5 else ec.rd(pos, f"{int(rng.integers(1, 12))}M{int(rng.integers(1, 30))}N30M")
        code, msg, _ = oracle_outcome(ec.G, [r, wide])
        seen.add(code)
        if code == -7:
            a, b = re.search(r"\((\d+) vs (\d+)\)", msg).groups()
            assert a == b == "0", (ops, msg)
        assert code == "ok" or code in (-2, -3, -4, -7, -13), (ops, msg)
    assert {"ok", -2, -3, -7} <= seen, seen
