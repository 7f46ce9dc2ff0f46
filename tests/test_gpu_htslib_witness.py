"""What the device writes for htslib to read, read by the reference's own htslib-1.3 (oracle/_ref/hts_witness, built where the
reference tree is and carried along with the working tree; tests/hts_witness.py): the BAM index of pjb_index_* and the BGZF
members of pjb_deflate_bgzf.  The `bamfilt` program's output is held to it in test_gpu_bamfilt.py::test_bamfilt_program."""
import gzip

import numpy as np
import pytest

import hts_witness as hts
import index_model as im
from portcullis_amd import ffi
from util_bam import BGZF_EOF, bam_header, read_bam, write_bam, write_bgzf

pytestmark = pytest.mark.gpu


def assert_same_answers(tmp_path, bam, refs, index_bytes, per_target=300):
    """htslib loads index_bytes and answers the region queries of test_oracle_htslib_witness.regions_for exactly as with the index
    it builds itself.  Returns the number of records the queries returned."""
    from test_oracle_htslib_witness import regions_for

    own, cand = str(tmp_path / "htslib.bai"), str(tmp_path / "candidate.bai")
    hts.index(bam, own)
    open(cand, "wb").write(index_bytes)
    regions = regions_for(refs, per_target)
    want, got = hts.query(bam, own, regions), hts.query(bam, cand, regions)
    for (reg, a), (_, b) in zip(got, want):
        assert a == b, reg
    return sum(len(hits) for _, hits in want)


def test_device_index_serves_htslib(tmp_path):
    """pjb_index_* over the mixed input at block size 4096, in pieces of 50 blocks: 1 200 queries."""
    from test_gpu_bam_index import device_bai

    reads = im.mixed_reads()
    assert 4_500 < len(reads) < 4_700
    p = str(tmp_path / "m.bam")
    write_bam(p, im.MIXED_REFS, reads, block_size=4096, write_index=False)
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as ctx:
        got, res = device_bai(ctx, p, len(im.MIXED_REFS), 50)
    assert res["n_records"] == len(reads)
    assert assert_same_answers(tmp_path, p, im.MIXED_REFS, got) > 50_000


@pytest.mark.parametrize("block_bytes", [0xFF00, 4096])
def test_device_deflate_is_a_bam_to_htslib(tmp_path, block_bytes):
    """A BAM stream -- util_bam's header and 2 000 records shaped like test_gpu_deflate._bam_like's -- through pjb_deflate_bgzf, the
    EOF block behind it: htslib finds the EOF marker and reads the records util_bam.read_bam reads from the same stream in zlib's
    members."""
    from test_gpu_deflate import _bam_like
    from test_oracle_htslib_witness import assert_records

    refs = [("chr1", 200_000), ("chr2", 200_000), ("chr3", 200_000)]
    stream = bam_header(refs) + _bam_like(np.random.default_rng(9), 2000)
    with ffi.Context(0, "UNKNOWN") as ctx:
        blob, sizes = ctx.deflate_bgzf(stream, block_bytes)
    assert len(sizes) == (len(stream) + block_bytes - 1) // block_bytes and len(sizes) > (1 if block_bytes == 4096 else 0)
    dev, ref = str(tmp_path / "device.bam"), str(tmp_path / "zlib.bam")
    open(dev, "wb").write(blob + BGZF_EOF)
    write_bgzf(ref, stream, block_bytes)
    assert gzip.open(dev, "rb").read() == stream
    assert hts.eof(dev) == 1
    want_refs, want = read_bam(ref)
    got_refs, got = hts.records(dev)
    assert got_refs == want_refs == refs and len(got) == len(want) == 2000
    recs = assert_records(dev)            # field by field: read_bam of the device's file against htslib on the same file ...
    for a, b in zip(recs, want):          # ... and read_bam of zlib's file says the same
        assert {k: (v.tobytes() if hasattr(v, "tobytes") else v) for k, v in a.items()} == \
               {k: (v.tobytes() if hasattr(v, "tobytes") else v) for k, v in b.items()}
    assert hts.eof(ref) == 1 and all(r["xs"] == "+" for r in recs)
