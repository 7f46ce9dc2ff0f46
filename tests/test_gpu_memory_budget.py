"""The context's device-memory books and its limit (pjb_memory_info, pjb_set_option "mem_limit"): `held` is the sum of the
categories wherever it is read; PJB_ERR_NOMEM from a submit call is retryable -- the target and the books are as they were, and
the same call succeeds once a chain has been collected --; what the context holds without needing it is released before a
request is refused; and targets run under a limit give the oracle's rows.

Targets of 200 - 300 fuzz reads on 12 - 15 kb genomes.  A target's records sit in a slab of 128 MB (the library's quantum), so a
limit of "what is held now + 1 KB" is short by a slab whatever the target's size."""
import pytest

from fuzzgen import make_reads
from parity import assert_rows_equal, region_equal
from util_bam import read_bam, records_to_batch, write_bam

pytestmark = pytest.mark.gpu

CATEGORIES = ("genomes", "slabs_open", "slabs_pooled", "staging", "scratch", "rows", "other")
# (target, reads, bases): the first is the largest in every respect, so that a later target's buffers never have to grow
SHAPES = ((0, 300, 15000), (1, 250, 13000), (2, 200, 12000))


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi
    assert ffi.device_count() >= 1, "no HIP device visible"
    return ffi


@pytest.fixture(scope="module")
def targets(tmp_path_factory):
    """Three targets in one BAM, with the oracle's rows -- computed once, shared by every test, never changed:
    [(genome bytes, batch, oracle rows, oracle region, BGZF bytes from the target's first block on, offset of its first record)]."""
    from oracle import oracle
    from test_gpu_ingest import bam_targets
    refs, reads, genomes = [], [], []
    for tid, n, glen in SHAPES:
        genome, rr = make_reads(70 + tid, n_reads=n, glen=glen)
        for r in rr:
            r["tid"] = tid
            if r.get("mtid", -1) >= 0:
                r["mtid"] = tid
        refs.append((f"chr{tid + 1}", len(genome)))
        genomes.append(genome.encode() if isinstance(genome, str) else genome)
        reads += rr
    path = str(tmp_path_factory.mktemp("membudget") / "in.bam")
    write_bam(path, refs, reads, block_size=4096)
    raw, _, first = bam_targets(path)
    _, recs = read_bam(path)
    out = []
    for tid, _, _ in SHAPES:
        batch = records_to_batch([r for r in recs if r["tid"] == tid])
        orows, oreg = oracle.find_juncs(tid, len(genomes[tid]), genomes[tid], batch, "UNKNOWN")
        coff, uoff = first[tid]
        out.append((genomes[tid], batch, orows, oreg, raw[coff:], uoff))
    assert sum(len(t[2]) for t in out) > 10
    return out


def info(ctx, seen=None):
    """memory_info, checked: held is the sum of the categories, the peak is not below it."""
    m = ctx.memory_info()
    assert m["held"] == sum(m[k] for k in CATEGORIES), m
    assert m["peak_held"] >= m["held"], m
    assert m["hip_total"] >= m["hip_free"] > 0, m
    if seen is not None:
        seen.append(m["held"])
    return m


def books(m):
    """what must read the same before and after a call that failed (the device's own free memory is other processes' too)"""
    return {k: v for k, v in m.items() if k not in ("hip_free", "hip_total")}


def fresh(ctx, targets, upload=(0, 1, 2)):
    ctx.set_refs([len(t[0]) for t in targets])
    for tid in upload:
        ctx.upload_contig(tid, targets[tid][0])


def submit(ctx, route, targets, tid):
    _, batch, _, _, comp, uoff = targets[tid]
    if route == "submit_batch":
        ctx.submit_batch(tid, batch)
    elif route == "submit_bam":
        assert ctx.submit_bam(tid, comp, uoff) == batch.n
    else:
        assert ctx.submit_bam_pieces(tid, comp, uoff, [3000, 701]) == batch.n


def check_rows(rows, regs, targets, tids):
    for tid in tids:
        assert_rows_equal(rows[rows["refid"] == tid], targets[tid][2])
        region_equal(regs[tid], targets[tid][3])


def test_accounting(ffi, targets):
    seen = []
    with ffi.Context(0) as ctx:
        m = info(ctx, seen)
        assert m["held"] == 0 and m["limit"] == 0
        fresh(ctx, targets, upload=(0,))
        m = info(ctx, seen)
        assert m["genomes"] >= len(targets[0][0]) and m["slabs_open"] == 0 and m["slabs_pooled"] == 0
        ctx.submit_batch(0, targets[0][1])
        m = info(ctx, seen)
        assert m["slabs_open"] > 0 and m["slabs_pooled"] == 0
        ctx.finish_contig_begin(0)
        m = info(ctx, seen)
        assert m["slabs_open"] > 0 and m["scratch"] > 0
        with pytest.raises(ffi.PjbError) as e:  # refused while a chain is queued, like the other options
            ctx.set_option("mem_limit", 1 << 30)
        assert not e.value.retryable
        assert info(ctx)["limit"] == 0
        reg = ctx.finish_contig_end(0)
        rows = ctx.collect()
        m = info(ctx, seen)
        assert m["slabs_open"] == 0 and m["slabs_pooled"] > 0 and m["rows"] > 0
        assert m["peak_held"] >= max(seen)  # at least every `held` seen
        check_rows(rows, {0: reg}, targets, (0,))
        ctx.clear_rows()
        ctx.release_contig(0)
        m = info(ctx, seen)
        assert m["slabs_open"] == 0 and m["slabs_pooled"] > 0
        assert m["peak_held"] == m["held"]  # (clear_rows starts the peak again)
        ctx.set_option("mem_limit", 12345)
        assert info(ctx)["limit"] == 12345
        # a round trip brings `held` back to what it was: everything the second target needs is there already
        before = books(m)
        ctx.set_option("mem_limit", 0)
        ctx.upload_contig(0, targets[0][0])
        ctx.submit_batch(0, targets[0][1])
        assert info(ctx)["slabs_open"] > 0
        ctx.finish_contig(0)
        ctx.clear_rows()
        ctx.release_contig(0)
        after = books(info(ctx, seen))
        assert after == dict(before, limit=0), (before, after)


@pytest.mark.parametrize("route", ["submit_batch", "submit_bam", "submit_bam_pieces"])
def test_nomem_is_retryable(ffi, targets, route):
    with ffi.Context(0) as probe:
        fresh(probe, targets)
        submit(probe, route, targets, 0)
        probe.finish_contig_begin(0)
        H = info(probe)["held"]
        probe.finish_contig_end(0)
    with ffi.Context(0) as ctx:
        fresh(ctx, targets)
        ctx.set_option("mem_limit", H + 1024)
        submit(ctx, route, targets, 0)
        ctx.finish_contig_begin(0)
        before = info(ctx)
        assert before["held"] == H and before["limit"] == H + 1024
        with pytest.raises(ffi.PjbError) as e:
            submit(ctx, route, targets, 1)
        assert e.value.code == ffi.ERR_NOMEM and e.value.retryable, e.value
        for word in ("wanted", "held", "limit %d" % (H + 1024)):
            assert word in str(e.value), e.value
        after = info(ctx)
        assert books(after) == books(before), (before, after)
        # the same call again with nothing freed: the library now tries slabs of the exact size, which this limit does not hold either
        with pytest.raises(ffi.PjbError) as e:
            if route == "submit_bam_pieces":
                ctx.bam_end(1, targets[1][5])
            else:
                submit(ctx, route, targets, 1)
        assert e.value.code == ffi.ERR_NOMEM and e.value.retryable
        assert books(info(ctx)) == books(before)
        regs = {0: ctx.finish_contig_end(0)}
        ctx.collect()
        assert info(ctx)["slabs_pooled"] > 0
        if route == "submit_bam_pieces":  # only pjb_bam_end is repeated: the pieces and their inflate are still the context's
            assert ctx.bam_end(1, targets[1][5]) == targets[1][1].n
        else:
            submit(ctx, route, targets, 1)
        regs[1] = ctx.finish_contig(1)
        rows = ctx.collect()
        check_rows(rows, regs, targets, (0, 1))
        m = info(ctx)
        assert m["peak_held"] <= m["limit"]


def test_release_before_refusal(ffi, targets):
    with ffi.Context(0) as ctx:
        fresh(ctx, targets, upload=(0,))
        ctx.submit_batch(0, targets[0][1])
        regs = {0: ctx.finish_contig(0)}
        m = info(ctx)
        assert m["slabs_pooled"] > 0 and m["slabs_open"] == 0
        ctx.set_option("mem_limit", m["held"] + len(targets[1][0]) // 2)
        ctx.upload_contig(1, targets[1][0])  # does not fit beside the pooled slab: the slab goes, the upload succeeds
        m = info(ctx)
        assert m["slabs_pooled"] == 0 and m["held"] <= m["limit"]
        ctx.submit_batch(1, targets[1][1])
        regs[1] = ctx.finish_contig(1)
        check_rows(ctx.collect(), regs, targets, (0, 1))
        m = info(ctx)
        assert m["peak_held"] <= m["limit"]


def test_group_flow(ffi, targets):
    tids = [0, 1, 2]
    # what one target's records take, as an unlimited context sees it
    largest = 0
    with ffi.Context(0) as probe:
        fresh(probe, targets)
        for tid in tids:
            probe.submit_batch(tid, targets[tid][1])
            largest = max(largest, info(probe)["slabs_open"])
            probe.finish_contig(tid)
        roomy = info(probe)["peak_held"] * 4
    assert largest > 0
    with ffi.Context(0) as ctx:
        # one group under a limit that holds all three
        fresh(ctx, targets)
        ctx.set_option("mem_limit", roomy)
        for tid in tids:
            ctx.submit_batch(tid, targets[tid][1])
        assert info(ctx)["slabs_open"] >= largest
        ctx.finish_group_begin(tids)
        regs = ctx.finish_group_end(tids)
        check_rows(ctx.collect(), regs, targets, tids)
        m = info(ctx)
        assert m["peak_held"] <= roomy and m["slabs_open"] == 0
    with ffi.Context(0) as ctx:
        # The same three one by one, under a limit that holds ONE target's records beside the fixed costs.  "Held with genomes only" is
        # read where the genomes are the only thing of the targets that the context holds -- a first target has been run, collected
        # and cleared, so that the chains' scratch and the row table (fixed costs: the formula leaves them 4 096 bytes otherwise)
        # are in it; the slab that run left in the pool is records, not a fixed cost, and is taken out again.
        fresh(ctx, targets)
        ctx.submit_batch(0, targets[0][1])
        ctx.finish_contig(0)
        ctx.clear_rows()
        m = info(ctx)
        assert m["slabs_pooled"] == largest and m["slabs_open"] == 0
        limit = m["held"] - m["slabs_pooled"] + largest + 4096
        ctx.set_option("mem_limit", limit)
        regs = {}
        for tid in tids:
            ctx.submit_batch(tid, targets[tid][1])
            regs[tid] = ctx.finish_contig(tid)  # (collected before the next target's records come)
            ctx.collect()
            assert info(ctx)["slabs_open"] == 0
        check_rows(ctx.collect(), regs, targets, tids)
        m = info(ctx)
        assert m["limit"] == limit and m["peak_held"] <= limit
        assert m["peak_held"] > limit - largest  # (the limit was in reach: the one slab it holds was held)
        assert m["largest_target_bytes"] == largest and m["largest_target"] in tids
        # ... and it holds no second target's records: with target 0 open, target 1 is refused, retryably, and nothing changes
        ctx.clear_rows()
        ctx.submit_batch(0, targets[0][1])
        before = books(info(ctx))
        with pytest.raises(ffi.PjbError) as e:
            ctx.submit_batch(1, targets[1][1])
        assert e.value.code == ffi.ERR_NOMEM and e.value.retryable
        assert books(info(ctx)) == before
        regs = {0: ctx.finish_contig(0)}
        ctx.submit_batch(1, targets[1][1])
        regs[1] = ctx.finish_contig(1)
        ctx.submit_batch(2, targets[2][1])
        regs[2] = ctx.finish_contig(2)
        check_rows(ctx.collect(), regs, targets, tids)
        assert info(ctx)["peak_held"] <= limit
