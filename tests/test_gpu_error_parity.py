"""Device error codes and ordinals against the oracle, fault by fault (through ctypes -> C ABI).

The junc kernels turn every condition under which the reference throws into an error word, min over (alignment ordinal << 8 |
-code); pjb_finish_* turns the word into a PJB_ERR_* code and "... (alignment ordinal N on target T)".  This file pins, for the
catalogue of tests/error_cases.py: the code (the oracle's), the ordinal (the faulty read's -- at the seams of k1_count's tiles,
threads and batches, and inside a group), the rule "the lowest ordinal wins", that a context survives a failed chain, and that
the device ingest route and the program report the same."""
import os
import re
import subprocess

import numpy as np
import pytest

import error_cases as ec
from extra_util import add_names, assert_extra_equal, batch_with_names, oracle_extra
from fuzzgen import make_reads, to_batch
from parity import assert_rows_equal, region_equal
from portcullis_amd.records import ReadBatch

pytestmark = pytest.mark.gpu

MSG = re.compile(r"\(alignment ordinal (\d+) on target (-?\d+)\)")
N_SMALL = 9  # MAX_QUEUED + 1 clean targets
T_BG, T_G = 1, N_SMALL + 1  # targets: small 0 | the background | small 1 .. 8 | the catalogue's contig
SMALL_TIDS = [0] + list(range(2, N_SMALL + 1))


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi
    assert ffi.device_count() >= 1, "no HIP device visible"
    assert ffi.MAX_QUEUED + 1 == N_SMALL
    return ffi


def failure(ffi, call):
    """(code, ordinal, target, message) of the PjbError `call` raises."""
    with pytest.raises(ffi.PjbError) as e:
        call()
    m = MSG.search(str(e.value))
    assert m, str(e.value)
    return e.value.code, int(m.group(1)), int(m.group(2)), str(e.value)


def oracle_code(orc, tid, genome, reads, orientation):
    try:
        orc.find_juncs(tid, len(genome), genome, ReadBatch.from_reads(reads), orientation)
    except orc.OracleError as e:
        return e.code
    return "ok"


class World:
    """The targets every test here uses, their oracle rows, and one context per orientation that the tests share on purpose: a
    chain that fails must leave it fit for the next one."""

    def __init__(self, ffi, orc):
        self.genome = {}
        self.reads = {}
        for k, tid in enumerate(SMALL_TIDS):
            self.genome[tid], self.reads[tid] = make_reads(7200 + k, glen=8000, n_reads=300, paired=True)
        self.genome[T_BG], self.reads[T_BG] = ec.background()
        self.genome[T_G], self.reads[T_G] = ec.G, [ec.CLEAN]
        self.refs = [len(self.genome[t]) for t in range(T_G + 1)]
        self.batch = {t: to_batch(r) for t, r in self.reads.items()}
        self._want = {}
        self.ctx = {}
        for ori in ("UNKNOWN", "FR"):
            self.ctx[ori] = self.context(ffi, ori)

    def context(self, ffi, orientation, flags=0):
        ctx = ffi.Context(0, orientation, flags=flags)
        ctx.set_refs(self.refs)
        for t, g in self.genome.items():
            ctx.upload_contig(t, g.encode())
        return ctx

    def want(self, orc, tid, orientation):
        """(rows, region) of the oracle for the clean reads of `tid`: computed once, never changed."""
        if (tid, orientation) not in self._want:
            self._want[tid, orientation] = orc.find_juncs(tid, self.refs[tid], self.genome[tid], self.batch[tid], orientation)
        return self._want[tid, orientation]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def world(ffi, orc):
    w = World(ffi, orc)
    yield w
    w.close()


def run(ctx, tid, batches):
    ctx.clear_rows()
    for b in batches:
        ctx.submit_batch(tid, b)
    reg = ctx.finish_contig(tid)
    return ctx.collect(), reg


def check_clean(world, orc, ctx, tid, orientation):
    rows, reg = run(ctx, tid, [world.batch[tid]])
    orows, oreg = world.want(orc, tid, orientation)
    region_equal(reg, oreg)
    assert_rows_equal(rows, orows)
    return orows


# ------------------------------------------------------------------ code and ordinal, fault by fault
@pytest.mark.parametrize("orientation", ["UNKNOWN", "FR"])
@pytest.mark.parametrize("name", [f.name for f in ec.CATALOGUE])
def test_catalogue_code_and_ordinal(ffi, orc, world, name, orientation):
    f = ec.BY_NAME[name]
    ctx = world.ctx[orientation]
    code, ordinal, target, msg = failure(ffi, lambda: run(ctx, T_G, [ReadBatch.from_reads(f.reads)]))
    if f.oracle is not None:
        assert oracle_code(orc, T_G, ec.G, f.reads, orientation) == f.oracle
    assert code == f.code, msg
    assert target == T_G, msg
    if f.at == ec.WINDOW:
        assert ordinal in ec.WINDOW_ORDINALS, msg
    else:
        assert ordinal == f.at, msg


def test_negative_position_is_taken_by_the_library(ffi, orc, world):
    """ANCHOR_LEN's only route is a record that starts before its contig: the ABI does not refuse it, a clean one gives rows."""
    reads = [dict(pos=-5, cigar="50M", seq=None, xs="+"), ec.rd(1000, "50M100N50M")]
    rows, reg = run(world.ctx["UNKNOWN"], T_G, [ReadBatch.from_reads(reads)])
    orows, oreg = orc.find_juncs(T_G, len(ec.G), ec.G, ReadBatch.from_reads(reads), "UNKNOWN")
    region_equal(reg, oreg)
    assert_rows_equal(rows, orows)


# ------------------------------------------------------------------ position sweep
def test_background_rows(orc, world):
    """The background alone gives the oracle's rows on the contexts of the sweep: a planted fault is the only one."""
    for ori in ("UNKNOWN", "FR"):
        assert len(check_clean(world, orc, world.ctx[ori], T_BG, ori)) > 10
    assert world.batch[T_BG].n == ec.BACKGROUND_READS


def sweep_ordinals(kind):
    return [k for k in ec.SWEEP_ORDINALS if k >= ec.PLANTS[kind][3]]


def expected_code(orc, world, kind, bad, orientation="FR"):
    _, code, in_oracle, _ = ec.PLANTS[kind]
    if in_oracle:
        assert oracle_code(orc, T_BG, world.genome[T_BG], bad, orientation) == code
    return code


@pytest.mark.parametrize("kind", sorted(ec.PLANTS))
def test_position_sweep(ffi, orc, world, kind):
    """One batch of two whole tiles and a partial one: k1_count's whole-tile path (four reads a thread) and its rounds path, the
    thread, wavefront and tile seams."""
    ctx = world.ctx["FR"]
    for k in sweep_ordinals(kind):
        bad = ec.plant(world.genome[T_BG], world.reads[T_BG], kind, k)
        want = expected_code(orc, world, kind, bad)
        code, ordinal, target, msg = failure(ffi, lambda: run(ctx, T_BG, [to_batch(bad)]))
        assert (code, ordinal, target) == (want, k, T_BG), (k, msg)
    check_clean(world, orc, ctx, T_BG, "FR")


@pytest.mark.parametrize("cut", [1000, 1024])
@pytest.mark.parametrize("kind", sorted(ec.PLANTS))
def test_seam_in_two_batches(ffi, orc, world, kind, cut):
    """The same reads in two batches: ordinals run on through DevBatch::base, the first read of batch two is compared with the
    last of batch one (prev_pos)."""
    ctx = world.ctx["FR"]
    for k in (1023, 1024):
        bad = to_batch(ec.plant(world.genome[T_BG], world.reads[T_BG], kind, k))
        want = ec.PLANTS[kind][1]
        code, ordinal, target, msg = failure(ffi, lambda: run(ctx, T_BG, [bad.slice(0, cut), bad.slice(cut, bad.n)]))
        assert (code, ordinal, target) == (want, k, T_BG), (k, msg)
    clean = world.batch[T_BG]
    rows, reg = run(ctx, T_BG, [clean.slice(0, cut), clean.slice(cut, clean.n)])
    region_equal(reg, world.want(orc, T_BG, "FR")[1])
    assert_rows_equal(rows, world.want(orc, T_BG, "FR")[0])


def run_group(ctx, world, tids, batches):
    ctx.clear_rows()
    for t in tids:
        ctx.submit_batch(t, batches[t])
    ctx.finish_group_begin(tids)
    regs = ctx.finish_group_end(tids)
    return ctx.collect(), regs


@pytest.mark.parametrize("kind", sorted(ec.PLANTS))
def test_seam_inside_a_group(ffi, orc, world, kind):
    """The faulty target as the second member of a three-member group: the ordinal runs through the whole group (the members
    before it count), the message names the group's first target.  A member's first read before the previous member's last is
    not unsorted: the clean group gives every member's oracle rows."""
    ctx = world.ctx["FR"]
    tids = [0, T_BG, 2]
    assert world.reads[0][-1]["pos"] > world.reads[T_BG][0]["pos"] and world.reads[T_BG][-1]["pos"] > world.reads[2][0]["pos"]
    rows, regs = run_group(ctx, world, tids, world.batch)
    for t in tids:
        region_equal(regs[t], world.want(orc, t, "FR")[1])
        assert_rows_equal(rows[rows["refid"] == t], world.want(orc, t, "FR")[0])
    before = world.batch[0].n
    for k in (1023, 1024):
        bad = ec.plant(world.genome[T_BG], world.reads[T_BG], kind, k)
        want = expected_code(orc, world, kind, bad)  # (target by target: the other two members are clean, see above)
        batches = dict(world.batch)
        batches[T_BG] = to_batch(bad)
        code, ordinal, target, msg = failure(ffi, lambda: run_group(ctx, world, tids, batches))
        assert (code, ordinal, target) == (want, before + k, tids[0]), (k, msg)


# ------------------------------------------------------------------ the lowest ordinal wins
FAR, NEAR = (100, 1500), (10, 12)  # more than a tile apart; two threads of one wavefront


@pytest.mark.parametrize("first,second", [
    ("QUERY_RANGE", "BAD_XS"), ("BAD_XS", "QUERY_RANGE"),        # k1_count after / before k4b_generic
    ("ZERO_LEN_OP", "UNSORTED"), ("UNSORTED", "ZERO_LEN_OP"),
    ("NO_SEQ", "ZERO_LEN_OP"), ("ZERO_LEN_OP", "NO_SEQ"),        # NO_SEQ against an anchor_side code
    ("BAD_XS", "UNSORTED"), ("QUERY_RANGE", "ZERO_LEN_OP"),      # two faults of one kernel
])
@pytest.mark.parametrize("where", [FAR, NEAR], ids=["a_tile_apart", "one_wavefront"])
def test_lowest_ordinal_wins(ffi, orc, world, first, second, where):
    """Two faults with different codes: the device reports the lower ordinal with that read's code, whichever kernel of the chain
    finds it -- the later kernels still run after an earlier one has flagged.  (The oracle follows the reference's order -- all
    reads first, then junction by junction -- and may name the other one: it only has to raise.)"""
    k1, k2 = where
    bad = ec.plant(world.genome[T_BG], ec.plant(world.genome[T_BG], world.reads[T_BG], first, k1), second, k2)
    if ec.PLANTS[first][2] and ec.PLANTS[second][2]:
        assert oracle_code(orc, T_BG, world.genome[T_BG], bad, "FR") in (ec.PLANTS[first][1], ec.PLANTS[second][1])
    code, ordinal, target, msg = failure(ffi, lambda: run(world.ctx["FR"], T_BG, [to_batch(bad)]))
    assert (code, ordinal) == (ec.PLANTS[first][1], k1), msg


@pytest.mark.parametrize("kind,k", [("BAD_XS", 1500), ("ZERO_LEN_OP", 5), ("NO_SEQ", ec.BACKGROUND_READS - 1)])
def test_read_level_fault_beats_window_fault(ffi, orc, world, kind, k):
    """k5_finalize reports under sentinel ordinals above every read's: a read-level fault always wins."""
    genome = world.genome[T_BG]
    tail = ec.window_fault_read(len(genome))
    alone = failure(ffi, lambda: run(world.ctx["FR"], T_BG, [to_batch(world.reads[T_BG] + [tail])]))
    assert alone[0] == -10 and alone[1] in ec.WINDOW_ORDINALS, alone
    bad = ec.plant(genome, world.reads[T_BG], kind, k) + [tail]
    if ec.PLANTS[kind][2]:
        assert oracle_code(orc, T_BG, genome, bad, "FR") in (ec.PLANTS[kind][1], -10)
    code, ordinal, target, msg = failure(ffi, lambda: run(world.ctx["FR"], T_BG, [to_batch(bad)]))
    assert (code, ordinal) == (ec.PLANTS[kind][1], k), msg


def test_two_phase_example(ffi, orc, world):
    """Read 0 = 50M100N (NO_PRESENCE, which the reference finds when it processes the junction), read 1 with XS '*' (which it
    finds in its read loop): the oracle reports -1 on read 1, the device -2 on ordinal 0 -- k4b_generic still reaches its
    set_error after k1_count has flagged."""
    reads = [dict(pos=1000, cigar="50M100N", seq=ec.G[1000:1050], xs="+"), dict(pos=1010, cigar="50M", seq=None, xs="*")]
    assert oracle_code(orc, T_G, ec.G, reads, "UNKNOWN") == -1
    code, ordinal, target, msg = failure(ffi, lambda: run(world.ctx["UNKNOWN"], T_G, [ReadBatch.from_reads(reads)]))
    assert (code, ordinal, target) == (-2, 0, T_G), msg


# ------------------------------------------------------------------ the context survives
def faulty_background(world, stage):
    """(reads, code) of a background with one fault that the named stage of the chain detects."""
    if stage == "k1_count":
        return ec.plant(world.genome[T_BG], world.reads[T_BG], "BAD_XS", 1024), -1
    if stage == "k4b_generic":
        return ec.plant(world.genome[T_BG], world.reads[T_BG], "QUERY_RANGE", 1024), -4
    assert stage == "k5_finalize"
    return world.reads[T_BG] + [ec.window_fault_read(len(world.genome[T_BG]))], -10


def clean_rows(world, orc, tids, orientation):
    return np.concatenate([world.want(orc, t, orientation)[0] for t in tids])


@pytest.mark.parametrize("stage", ["k1_count", "k4b_generic", "k5_finalize"])
def test_context_survives(ffi, orc, world, stage):
    """After a failed chain, MAX_QUEUED + 1 clean targets -- the failed chain's slot is used again --, one by one and queued
    eight deep: every clean target's rows and region are the oracle's, and the table holds exactly the clean rows (the error
    word and the list counters are restored by the chain itself)."""
    bad, want = faulty_background(world, stage)
    bad = to_batch(bad)
    ori = "UNKNOWN"
    with world.context(ffi, ori) as ctx:
        for depth in (1, ffi.MAX_QUEUED):
            ctx.clear_rows()
            ctx.submit_batch(T_BG, bad)
            assert failure(ffi, lambda: ctx.finish_contig(T_BG))[0] == want
            queued, regs = [], {}
            for t in SMALL_TIDS:
                ctx.submit_batch(t, world.batch[t])
                ctx.finish_contig_begin(t)
                queued.append(t)
                if len(queued) >= depth:
                    done = queued.pop(0)
                    regs[done] = ctx.finish_contig_end(done)
            for t in queued:
                regs[t] = ctx.finish_contig_end(t)
            for t in SMALL_TIDS:
                region_equal(regs[t], world.want(orc, t, ori)[1])
                assert regs[t]["n_junctions"] == len(world.want(orc, t, ori)[0])
            rows = ctx.collect()
            assert list(dict.fromkeys(rows["refid"].tolist())) == SMALL_TIDS
            assert_rows_equal(rows, clean_rows(world, orc, SMALL_TIDS, ori))


@pytest.mark.parametrize("stage", ["k1_count", "k4b_generic", "k5_finalize"])
def test_faulty_chain_between_two_clean_ones(ffi, orc, world, stage):
    """finish_contig_begin x 3, then the ends in order: the neighbours are intact, the middle _end raises the code."""
    bad, want = faulty_background(world, stage)
    ori = "FR"
    with world.context(ffi, ori) as ctx:
        ctx.clear_rows()
        ctx.submit_batch(0, world.batch[0])
        ctx.submit_batch(T_BG, to_batch(bad))
        ctx.submit_batch(2, world.batch[2])
        for t in (0, T_BG, 2):
            ctx.finish_contig_begin(t)
        region_equal(ctx.finish_contig_end(0), world.want(orc, 0, ori)[1])
        code, ordinal, target, msg = failure(ffi, lambda: ctx.finish_contig_end(T_BG))
        assert (code, target) == (want, T_BG), msg
        region_equal(ctx.finish_contig_end(2), world.want(orc, 2, ori)[1])
        assert_rows_equal(ctx.collect(), clean_rows(world, orc, [0, 2], ori))
        check_clean(world, orc, ctx, T_BG, ori)  # and the failed target itself, clean this time


def test_extra_context_survives(ffi, orc):
    """A PJB_FLAG_EXTRA context: the first target fails in k4b_generic, the extra columns of the clean targets behind it equal
    the oracle's for a file without the failed target's records."""
    rng = np.random.default_rng(8)
    f = ec.BY_NAME["sequence_shorter_than_cigar_with_deletion"]
    bad = [dict(r) for r in f.reads]
    pool = add_names(bad, rng, "bad")
    contigs = [(ec.G, None)]
    for k in range(2):
        genome, reads = make_reads(7300 + k, glen=8000, n_reads=600)
        add_names(reads, rng, f"c{k}", pool)
        contigs.append((genome, reads))
    orows, _ = oracle_extra(orc, contigs, "UNKNOWN")
    with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_EXTRA) as ctx:
        ctx.set_refs([len(g) for g, _ in contigs])
        ctx.clear_rows()
        for tid, (genome, reads) in enumerate(contigs):
            ctx.upload_contig(tid, genome.encode())
            ctx.submit_batch(tid, batch_with_names(orc, bad if tid == 0 else reads))
            if tid == 0:
                code, ordinal, target, msg = failure(ffi, lambda: ctx.finish_contig(0))
                assert (code, ordinal, target) == (f.code, f.at, 0), msg
            else:
                ctx.finish_contig(tid)
        rows = ctx.collect()
        extra = ctx.extra_finish()
    assert_rows_equal(rows, orows)
    assert_extra_equal(rows, extra, orows)
    assert (extra["up_aln"] > 0).any() and (extra["coverage"] != 0).any()


# ------------------------------------------------------------------ device ingest route
@pytest.mark.parametrize("name,xs_tag", [("bad_xs_behind_a_clean_read", "*"), ("sequence_shorter_than_cigar_with_deletion", None),
                                         ("read_before_its_predecessor", None)])
def test_bam_route_reports_the_same(ffi, orc, world, tmp_path, name, xs_tag):
    """The same records as BAM bytes (pjb_submit_bam, and pjb_bam_begin / _piece / _end): code and ordinal as through submit_batch."""
    from test_gpu_ingest import bam_targets
    from util_bam import write_bam
    f = ec.BY_NAME[name]
    reads = [dict(r, tid=0, name=f"r{k}") for k, r in enumerate(f.reads)]
    if xs_tag is not None:
        reads[f.at]["xs"] = xs_tag  # an XS:A:* tag
    path = str(tmp_path / "fault.bam")
    write_bam(path, [("chrG", len(ec.G))], reads, write_index=False)
    raw, refs, first = bam_targets(path)
    coff, uoff = first[0]
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([len(ec.G)])
        ctx.upload_contig(0, ec.G.encode())
        ctx.clear_rows()
        ctx.submit_batch(0, ReadBatch.from_reads(reads))
        want = failure(ffi, lambda: ctx.finish_contig(0))[:3]
        assert want == (f.code, f.at, 0)
        ctx.clear_rows()
        assert ctx.submit_bam(0, raw[coff:], uoff) == len(reads)
        assert failure(ffi, lambda: ctx.finish_contig(0))[:3] == want
        ctx.clear_rows()
        assert ctx.submit_bam_pieces(0, raw[coff:], uoff, [64, 1000]) == len(reads)
        assert failure(ffi, lambda: ctx.finish_contig(0))[:3] == want


# ------------------------------------------------------------------ the program
def test_program_reports_code_text_and_ordinal(tmp_path):
    """`portcullis_amd junc` on a prepared directory whose BAM holds one anchor_side fault: non-zero exit, the condition's text and
    the ordinal on stderr; oracle/orc_bam2tab fails on the same file."""
    from test_gpu_host_cli import run_cli
    from util_bam import make_prep_dir
    f = ec.BY_NAME["sequence_shorter_than_cigar_with_deletion"]
    reads = [dict(r, tid=0, name=f"r{k}") for k, r in enumerate(f.reads)]
    prep = make_prep_dir(str(tmp_path / "prep"), [("chrG", len(ec.G))], [("chrG", ec.G)], reads)
    os.makedirs(str(tmp_path / "out"))
    p = run_cli(prep, str(tmp_path / "out" / "pc"), "-t", "1")
    assert p.returncode != 0, p.stdout[-1000:]
    assert "Can't extract cigar op sequence from query string" in p.stderr and f"alignment ordinal {f.at} on target 0" in p.stderr, p.stderr[-2000:]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "orc_bam2tab")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    q = subprocess.run([exe, prep, str(tmp_path / "cpu.tab"), "1", "UNKNOWN"], capture_output=True, text=True, timeout=120)
    assert q.returncode != 0 and "Can't extract cigar op sequence from query string" in q.stderr, q.stderr[-1000:]
