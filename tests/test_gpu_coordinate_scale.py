"""junc chains at chromosome-scale coordinates and with introns of 2^18 bases and more.

One sparse target of 2^28 + 12 325 bases (scale_util.big_genome: positions of 29 bits, a ragged last bitmap word and page), uploaded
through the host route, so that k0_upper / k0_encode / k0_encode2 run over more than 2^28 bases as well.  What the tests pin:
  the start bitmap's geometry: a start in bit 0 / 63 of a word, on a page edge, either side of the page ranks' scan tiles, in the
    first word, either side of 2^28, in the ragged last word -- on the run route, the radix route and the full-key chain;
  the exception channel at stretch 2^22 of its bitmap;
  OVF_KEYFMT without "weird" coordinates: an intron of 2^18 bases repeats the chain with wider keys, the context keeps the width,
    keys of 57 bits sort in more passes, and a group repeats as a group with the chain queued behind it taken back;
  the same through pjb_submit_bam, with raw keys (an alignment that leaves the target), with PJB_FLAG_EXTRA;
  either side of RES_FIELD_MAX (anchors of 0xfffff and 0x100000 bases), on a genome of its own.
Every row is compared with the oracle's; the route witnesses (repeats, repeat_reasons, sort_passes, generic_pairs, kernel names) show
that the code meant ran.  The read sets themselves are pinned by test_oracle_scale_inputs.py.  Each test prints its witnesses and wall
time (pytest -s)."""
import time

import numpy as np
import pytest

import scale_util as su
from parity import assert_rows_equal, region_equal

pytestmark = pytest.mark.gpu

KEYFMT, APART = su.KEYFMT, su.APART


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi
    return ffi


@pytest.fixture(scope="module")
def big():
    """The big target's bytes, built once: the same object goes to the oracle and to upload_contig."""
    return su.big_genome()


def witness(t):
    return {k: t[k] for k in ("repeats", "repeat_reasons", "sort_passes", "generic_pairs")}


def test_bitmap_geometry(ffi, orc, big):
    specs = su.geometry()
    batch = su.oracle_rows(orc, "geometry", big, specs)[0]

    def check(ctx, v, t, drows):
        assert t["repeats"] == 0 and t["repeat_reasons"] == 0, (v, t)
        if v["dense_ids"]:
            kt = ctx.kernel_timing()
            assert "kd_rank_pages" in kt and kt["kd_rank_pages"][0] >= 1, (v, sorted(kt))
        # the same chain again on this context: kd_reset wiped the bitmap, the page counts and the end slots back to rest
        ctx.clear_rows()
        ctx.submit_batch(0, batch)
        ctx.finish_contig(0)
        t2 = ctx.timing()
        assert t2["repeats"] == 0, (v, t2)
        assert ctx.collect().tobytes() == drows.tobytes(), v

    variants = [dict(dense_ids=1, run_sort=1), dict(dense_ids=1, run_sort=0), dict(dense_ids=0)]
    ts = su.run_variants(ffi, orc, "geometry", big, specs, variants, flags=ffi.FLAG_KERNEL_TIMING, check=check)
    for v, t in zip(variants, ts):
        print("geometry", v, witness(t), f"{t['wall_s']:.2f} s")
    assert ts[2]["sort_passes"] > ts[1]["sort_passes"] >= 1, ts  # (keys of 18 + 29 bits against junction ids, which have 32 at the most)


def test_exception_channel_far_out(ffi, orc, big):
    specs = su.exception_reads()
    b, orows, oreg = su.oracle_rows(orc, "exceptions", big, specs)
    assert orows["sum_mismatches"].sum() > 0   # (the planted letters lie under the anchors)
    t0 = time.perf_counter()
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([len(big)])
        ctx.upload_contig(0, big)
        raw = []
        for seq2 in (True, False):
            ctx.clear_rows()
            ctx.submit_batch(0, b, seq2=seq2)
            region_equal(ctx.finish_contig(0), oreg)
            rows = ctx.collect()
            assert_rows_equal(rows, orows)
            raw.append(rows.tobytes())
            print("exceptions seq2 =", seq2, witness(ctx.timing()))
        assert raw[0] == raw[1]
    print(f"exceptions {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("dense", [1, 0])
def test_key_width(ffi, orc, big, dense):
    """One context, tid 0 resubmitted after clear_rows(): a, b (262 143: still 18 bits), c (262 144: the chain repeats for its key
    format and nothing else), c again (the context kept the width), e (2^20, 2^24 + 5, 2^28 - 1: repeats again), a again on 57-bit keys."""
    t0 = time.perf_counter()
    seen = {}
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_option("dense_ids", dense)
        ctx.set_refs([len(big)])
        ctx.upload_contig(0, big)
        for step, name in (("a", "clusters"), ("b", "key_b"), ("c", "key_c"), ("d", "key_c"), ("e", "key_e"), ("f", "clusters")):
            b, orows, oreg = su.oracle_rows(orc, name, big, su.BIG_SETS[name]())
            ctx.clear_rows()
            ctx.submit_batch(0, b)
            region_equal(ctx.finish_contig(0), oreg)
            assert_rows_equal(ctx.collect(), orows)
            seen[step] = t = ctx.timing()
            print("key width, dense_ids", dense, "step", step, witness(t))
            if step in "abdf":
                assert t["repeats"] == 0 and t["repeat_reasons"] == 0, (step, t)
            else:
                assert t["repeats"] >= 1 and t["repeat_reasons"] == KEYFMT, (step, t)
    if not dense:
        assert seen["f"]["sort_passes"] > seen["a"]["sort_passes"], (seen["a"], seen["f"])
    print(f"key width, dense_ids {dense}: {time.perf_counter() - t0:.2f} s")


def test_ingest(ffi, orc, big, tmp_path):
    """Read set (e) as BAM bytes through pjb_submit_bam on a fresh context: the same rows, the same repeat."""
    from util_bam import write_bam
    specs = su.key_set("e")
    b, orows, oreg = su.oracle_rows(orc, "key_e", big, specs)
    reads = su.reads_of(big, specs)
    for k, r in enumerate(reads):
        r["tid"] = 0
        r["name"] = f"r{k}"
    path = str(tmp_path / "scale.bam")
    write_bam(path, [("big", su.L_BIG)], reads, write_index=False)
    raw = open(path, "rb").read()
    lens, first = ffi.bam_header(raw)
    assert lens == [su.L_BIG]
    t0 = time.perf_counter()
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs(lens)
        ctx.upload_contig(0, big)
        ctx.clear_rows()
        assert ctx.submit_bam(0, raw, first) == len(reads) == b.n
        region_equal(ctx.finish_contig(0), oreg)
        assert_rows_equal(ctx.collect(), orows)
        t = ctx.timing()
    print("ingest", witness(t), f"{time.perf_counter() - t0:.2f} s")
    assert t["repeats"] >= 1 and t["repeat_reasons"] == KEYFMT, t


def test_raw_keys_far_out(ffi, orc, big):
    """Read set (e) with alignments that run past the end of the target: coordinates outside it take the raw-key route (64-bit keys,
    no dense ids).
      Two that the reference clamps and accepts, through test_gpu_edge_cases.both and once more for the witnesses: the chain repeats
    for its key format alone and sorts in more passes than the next chain on this context, read set (e) alone on dense ids.
      test_gpu_groups' taken-apart member, 100 bases before the end as there: one fault, the same code on both sides.
      The same 40 bases before the end has two faults: its record holds 40 bases for 110 (QUERY_RANGE), and its intron starts behind
    the end (SPLICE_SITE_LEN, which the reference meets first).  test_gpu_error_parity pins the rule for that: the oracle only has to
    raise, the device names the read-level fault with the read's ordinal (both()'s equal codes are for inputs with one fault)."""
    import re

    from portcullis_amd.records import ReadBatch
    from test_gpu_edge_cases import both
    t0 = time.perf_counter()
    genome = big.decode()
    status, rows = both(ffi, orc, genome, su.reads_of(big, su.RAW_OK()))
    assert status == "ok" and len(rows) == len(su.expected(su.key_set("e"))) + 1
    b, orows, oreg = su.oracle_rows(orc, "raw_ok", big, su.RAW_OK())
    b_e, orows_e, oreg_e = su.oracle_rows(orc, "key_e", big, su.key_set("e"))
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([len(big)])
        drows, dreg = ffi.run_contig(ctx, 0, big, [b])
        t_raw = ctx.timing()
        region_equal(dreg, oreg)
        assert_rows_equal(drows, orows)
        ctx.clear_rows()
        ctx.submit_batch(0, b_e)
        region_equal(ctx.finish_contig(0), oreg_e)
        assert_rows_equal(ctx.collect(), orows_e)
        t_e = ctx.timing()
    print("raw keys: clamped and accepted", witness(t_raw), "then read set (e)", witness(t_e))
    assert t_raw["repeats"] >= 1 and t_raw["repeat_reasons"] == KEYFMT and t_raw["sort_passes"] > t_e["sort_passes"], (t_raw, t_e)

    status, codes = both(ffi, orc, genome, su.reads_of(big, su.key_set("e") + [su.OFF_END_NEAR]))
    print("raw keys: 100 bases before the end", status, codes)
    assert status == "error" and codes == (-7, -7)

    reads = su.reads_of(big, su.key_set("e") + [su.OFF_END])
    at = [r["pos"] for r in reads].index(su.OFF_END[0])
    batch = ReadBatch.from_reads(reads)
    with pytest.raises(orc.OracleError) as oerr:
        orc.find_juncs(0, len(big), big, batch, "UNKNOWN")
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([len(big)])
        with pytest.raises(ffi.PjbError) as derr:
            ffi.run_contig(ctx, 0, big, [batch])
    print("raw keys: 40 bases before the end: oracle", oerr.value.code, "device", derr.value)
    m = re.search(r"alignment ordinal (\d+) on target 0", str(derr.value))
    assert oerr.value.code == -8 and derr.value.code == -4 and m and int(m.group(1)) == at, (oerr.value, derr.value)
    print(f"raw keys {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("order", [(0, 1, 2), (1, 2, 0)], ids=["big_first", "big_last"])
def test_groups(ffi, orc, big, order):
    """The big target with read set (e) and two 30 kb targets as ONE chain on a fresh context (its first attempt plans 18 length bits),
    a fourth target queued behind it: the group is repeated as a group -- not taken apart --, the chain behind it is taken back, and
    grouped rows == singles' rows == oracle.  With the big target first the other members sit at virtual offsets beyond 2^28."""
    from fuzzgen import make_reads, to_batch
    want = {0: su.oracle_rows(orc, "key_e", big, su.key_set("e")) + (big,)}
    for tid, seed in ((1, 7101), (2, 7102), (3, 7103)):
        genome, reads = make_reads(seed, n_reads=1500)
        b = to_batch(reads)
        orows, oreg = orc.find_juncs(tid, len(genome), genome, b, "UNKNOWN")
        want[tid] = (b, orows, oreg, genome.encode())
    group = list(order)
    all_rows = np.concatenate([want[t][1] for t in group + [3]])
    t0 = time.perf_counter()
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([len(want[t][3]) for t in range(4)])
        for t in range(4):
            ctx.upload_contig(t, want[t][3])
        ctx.clear_rows()
        for t in range(4):
            ctx.submit_batch(t, want[t][0])
        ctx.finish_group_begin(group)
        ctx.finish_contig_begin(3)  # (queued behind the group: its rows went where the repeated group's belong)
        regs = ctx.finish_group_end(group)
        t = ctx.timing()
        print("group", group, witness(t))
        assert t["repeats"] >= 1 and t["repeat_reasons"] & KEYFMT and not t["repeat_reasons"] & APART, t
        r3 = ctx.finish_contig_end(3)
        grouped = ctx.collect()
        for tid in group:
            region_equal(regs[tid], want[tid][2])
        region_equal(r3, want[3][2])
        assert_rows_equal(grouped, all_rows)
        assert list(dict.fromkeys(grouped["refid"].tolist())) == group + [3]
        assert_rows_equal(grouped[grouped["refid"] == 3], want[3][1])
        # one by one, in the same order (the context has the width now)
        ctx.clear_rows()
        for tid in group + [3]:
            ctx.submit_batch(tid, want[tid][0])
            region_equal(ctx.finish_contig(tid), want[tid][2])
        singles = ctx.collect()
        assert_rows_equal(singles, all_rows)
        assert grouped.tobytes() == singles.tobytes()
    print(f"group {group}: {time.perf_counter() - t0:.2f} s")


def test_extra(ffi, orc, big):
    """A PJB_FLAG_EXTRA context over the geometry clusters, unspliced reads around some of them and the 2^20 intron: rows and extra
    columns against the oracle's calcExtraMetrics."""
    from extra_util import add_names, assert_extra_equal, batch_with_names, oracle_extra
    reads = su.reads_of(big, su.extra_set())
    add_names(reads, np.random.default_rng(29), "x", unmapped_frac=0.1)
    t0 = time.perf_counter()
    orows, _ = oracle_extra(orc, [(big, reads)])
    t_orc = time.perf_counter() - t0
    assert (orows["coverage"] != 0).any() and (orows["up_aln"] > 0).any() and (orows["down_aln"] > 0).any()  # (the columns are not idle)
    t0 = time.perf_counter()
    with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_EXTRA) as ctx:
        ctx.set_refs([len(big)])
        ctx.clear_rows()
        ctx.upload_contig(0, big)
        ctx.submit_batch(0, batch_with_names(orc, reads))
        ctx.finish_contig(0)
        t = ctx.timing()
        rows = ctx.collect()
        extra = ctx.extra_finish()
    print("extra", witness(t), f"oracle {t_orc:.2f} s, device {time.perf_counter() - t0:.2f} s")
    assert_rows_equal(rows, orows)
    assert_extra_equal(rows, extra, orows)


def test_anchor_edge(ffi, orc):
    """Anchors of 0xfffff bases are the last k1_emit finishes in closed form (RES_FIELD_MAX), anchors of 0x100000 go to k1_generic: left
    anchor, right anchor, the closed middle block of a two-intron read, each also with a substitution at the long anchor's first and
    last base.  pjb_timing.generic_pairs tells the two routes apart."""
    g = su.anchor_genome()
    seen = {}
    for a in su.ANCHORS:
        t, = su.run_variants(ffi, orc, f"anchor_{a:x}", g, su.anchor_specs(a), [dict()])
        seen[a] = t
        print(f"anchor {a:#x}", witness(t), f"generic_reads {t['generic_reads']}", f"{t['wall_s']:.2f} s")
    assert seen[0xfffff]["generic_pairs"] == 0, seen[0xfffff]
    assert seen[0x100000]["generic_pairs"] > 0, seen[0x100000]
