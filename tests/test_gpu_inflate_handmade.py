"""Device-side BGZF inflate (bgzf_decode + bgzf_resolve, pjb_ingest.hip.h) on streams that zlib's encoder never writes: the
hand-made corpus of tests/inflate_cases.py, through Context.inflate_bgzf.  test_gpu_ingest.py and test_gpu_deflate.py hold
the decoder on what zlib and the device deflater produce; the arithmetic this file is for lies elsewhere:
  bgzf_decode   three codes a trip within "4 ring words, 5 + 15 + 13 bits in the buffer" (15-bit literals, a 15-bit length code
                with 5 extra bits, a 15-bit distance code with 13: shape/depth15-*), canonical limits / adj / the 0x1ff slot mask
                on full 286 + 30 alphabets, a single distance code, none, an end-of-block-only set; block headers at every bit
                phase; every way to spell the code lengths; lanes that re-enter mid-wave beside lanes of quite other streams;
  bgzf_resolve  every (distance 1..40, length 3..258) through its three copy branches, chains of back-to-back 3-byte matches
                that each read the one before (serial: zlib would have written one long match), sources across matches, batches
                of 64 and windows of 1 024, matches at the edges of words, windows and the block, the 3-byte token store;
  both          every malformed header and symbol refused with PJB_ERR_BGZF (-22), the block named, the context usable after.
The expected bytes are deflate_writer.expand of the tokens; tests/test_deflate_writer.py holds corpus and writer against zlib."""
import numpy as np
import pytest

import inflate_cases
from deflate_writer import Bits, bgzf_member, expand, fixed_block
from util_bam import BGZF_EOF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from portcullis_amd import ffi
    assert ffi.device_count() >= 1
    with ffi.Context(0, "UNKNOWN") as c:
        yield c


@pytest.fixture(scope="module")
def accept():
    return inflate_cases.accept_cases()


@pytest.fixture(scope="module")
def refuse():
    return inflate_cases.refuse_cases()


def _member(case):
    return bgzf_member(case.payload, case.isize)


def _good():
    tokens = list(b"a good member, before and after! good") + [(258, 32)] * 3 + [(182, 5)]
    data = expand(tokens)
    assert len(data) == 993   # the next block's base is no multiple of anything
    b = Bits()
    fixed_block(b, tokens, True)
    return bgzf_member(b.bytes(), len(data)), data


def test_accept_cases_alone(ctx, accept):
    """Each case as the only member of a call (+ EOF), byte for byte what `expand` says."""
    assert len(accept) > 250 and sum(1 for c in accept if c.name.startswith("fuzz/")) == 200
    wrong = []
    for c in accept:
        out = ctx.inflate_bgzf(_member(c) + BGZF_EOF)
        if out != c.expected:
            n = min(len(out), len(c.expected))
            first = next((i for i in range(n) if out[i] != c.expected[i]), n)
            wrong.append(f"{c.name}: {len(out)} bytes for {len(c.expected)}, first difference at {first}")
    assert not wrong, "\n".join(wrong)


def test_refuse_cases_alone(ctx, refuse):
    """Each malformed stream, as the first block of a call and behind a good member (real bytes lie before its base then):
    PJB_ERR_BGZF; a good member still inflates afterwards."""
    from portcullis_amd import ffi
    good, data = _good()
    assert len(refuse) >= 29
    wrong = []
    for c in refuse:
        for index, comp in ((0, _member(c) + BGZF_EOF), (1, good + _member(c) + good + BGZF_EOF)):
            try:
                out = ctx.inflate_bgzf(comp)
                wrong.append(f"{c.name}: accepted, {len(out)} bytes")
            except ffi.PjbError as e:
                if e.code != -22 or f"BGZF block {index} (" not in str(e):  # (the decoder's verdict, not the container scan's)
                    wrong.append(f"{c.name}: {e}")
    assert not wrong, "\n".join(wrong)
    assert ctx.inflate_bgzf(good + BGZF_EOF) == data


@pytest.mark.parametrize("per_launch", [None, "64"])
def test_all_cases_mixed_in_one_call(ctx, accept, monkeypatch, per_launch):
    """Every accept case and 64 one-byte members in one call, in three orders: lanes of 78 bits a trip beside lanes of one bit
    a trip beside stored blocks, and -- with 64 lanes, one workgroup walking the whole list -- lanes that take up a new block
    while their neighbours are in the middle of theirs."""
    if per_launch:
        monkeypatch.setenv("PJB_INF_BLOCKS_PER_LAUNCH", per_launch)
    members = [(_member(c), c.expected) for c in accept]
    for k in range(64):
        b = Bits()
        fixed_block(b, [k + 48], True)
        members.append((bgzf_member(b.bytes(), 1), bytes([k + 48])))
    for seed in (1, 2, 3):
        order = np.random.default_rng(seed).permutation(len(members))
        comp = b"".join(members[int(i)][0] for i in order) + BGZF_EOF
        want = b"".join(members[int(i)][1] for i in order)
        out = ctx.inflate_bgzf(comp)
        assert len(out) == len(want)
        at = 0
        for i in order:  # (a failure names the member instead of showing two megabytes)
            n = len(members[int(i)][1])
            assert out[at:at + n] == members[int(i)][1], (seed, int(i), accept[int(i)].name if int(i) < len(accept) else "one byte")
            at += n


def test_error_names_the_block(ctx, accept, refuse):
    """One malformed member among a hundred good ones: the call fails and says which block it was."""
    from portcullis_amd import ffi
    good = [c for c in accept if c.isize < 20000][:100]
    assert len(good) == 100
    by = {c.name: c for c in refuse}
    for name, index in (("refuse/distance-past-start", 37), ("refuse/over-subscribed-literal-set", 0), ("refuse-isize/literal-past-isize", 99),
                        ("refuse/truncated-mid-code", 64)):
        members = [_member(c) for c in good]
        members.insert(index, _member(by[name]))
        with pytest.raises(ffi.PjbError) as e:
            ctx.inflate_bgzf(b"".join(members) + BGZF_EOF)
        assert e.value.code == -22 and f"BGZF block {index} " in str(e.value), (name, str(e.value))
    assert ctx.inflate_bgzf(b"".join(_member(c) for c in good) + BGZF_EOF) == b"".join(c.expected for c in good)
