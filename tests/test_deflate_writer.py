"""tests/deflate_writer.py and the corpus of tests/inflate_cases.py against zlib (no GPU): zlib inflates every accept
case to exactly what `expand` says, with `eof`, and refuses every refuse case that is zlib's to judge.  A mistake in the
writer or in a case therefore shows here, and cannot pass as a mistake of the decoders that the corpus is for
(tests/test_gpu_inflate_handmade.py, tests/test_host_fast_inflate.py)."""
import collections
import zlib

import numpy as np
import pytest

import deflate_writer as dw
import inflate_cases


@pytest.fixture(scope="module")
def corpus():
    cases, seconds = inflate_cases.build()
    print(f"corpus: {len(cases)} cases built in {seconds:.1f} s")
    assert seconds < 30  # "well under a minute"
    return cases


def _zlib(payload):
    """(bytes, eof, unused) -- or the zlib.error."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload) + d.flush()
    except zlib.error as e:
        return e
    return out, d.eof, d.unused_data


def test_corpus_groups(corpus):
    n = collections.Counter(c.name.split("/")[0] for c in corpus)
    print(dict(n))
    assert n["fuzz"] == inflate_cases.N_FUZZ == 200          # nothing skipped
    assert set(n) == set(inflate_cases.GROUPS)
    assert n["pairs"] >= 20 and n["chains"] == 5 and n["refuse"] >= 25 and n["refuse-isize"] >= 4
    pairs = [c for c in corpus if c.name.startswith("pairs/")]  # (the generator asserts that all 40 x 256 tokens are in them)
    assert sum(c.isize for c in pairs) > 40 * sum(range(3, 259))
    for c in corpus:
        dw.bgzf_member(c.payload, c.isize)                    # every case fits a member


def test_accept_cases_are_zlibs_too(corpus):
    accept = [c for c in corpus if c.expected is not None]
    assert len(accept) > 250
    for c in accept:
        r = _zlib(c.payload)
        assert not isinstance(r, zlib.error), (c.name, r)
        out, eof, unused = r
        assert eof, c.name
        assert out == c.expected, c.name
        assert len(out) == c.isize, c.name
        assert len(unused) == (9 if c.name == "blocks/trailing-bytes" else 0), c.name


def test_refuse_cases_are_refused_by_zlib(corpus):
    refuse = [c for c in corpus if c.name.startswith("refuse/")]
    for c in refuse:
        r = _zlib(c.payload)
        assert isinstance(r, zlib.error) or not r[1], (c.name, r)
    # the ISIZE cases: zlib takes the stream, and it does not yield ISIZE bytes
    mine = [c for c in corpus if c.name.startswith("refuse-isize/")]
    assert len(mine) >= 4
    for c in mine:
        out, eof, unused = _zlib(c.payload)
        assert eof and not unused and len(out) != c.isize, c.name


def test_case_geometry(corpus):
    """What the issue fixes about single cases."""
    by = {c.name: c for c in corpus}
    for name in ("chains/len3-dist3", "chains/len4-dist4", "chains/len3-dist6", "chains/len258-dist258", "chains/len3-dist1",
                 "edges/starts-63-1023-65533", "edges/far-matches-258-as-284", "edges/far-matches-258-as-285"):
        assert by[name].isize == 65536, name
    assert by["chains/len3-dist3"].expected[:6] == by["chains/len3-dist3"].expected[3:9]
    assert by["edges/match-at-isize-minus-3"].isize == 1000
    assert by["shape/eob-only"].isize == 0 and by["shape/eob-only"].expected == b""
    assert len(by["blocks/largest-stored"].payload) == dw.MAX_PAYLOAD and by["blocks/largest-stored"].isize == 65505
    assert len(by["shape/depth15-a"].payload) > 7000 * 73 // 8
    assert by["refuse/hclen-4"].payload[1] >> 5 == 0 and by["refuse/hclen-4"].payload[2] & 1 == 0  # the HCLEN field says 4


# ------------------------------------------------------------------------------------------------ the writer's parts
def test_bits_are_lsb_first_and_codes_msb_first():
    b = dw.Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.code(0b110, 3)     # first bit of the code lowest
    b.put(0x1ff, 9)
    assert b.bit_length == 15
    assert b.bytes() == bytes([0b11_011_10_1 & 0xff, 0b1111111])
    b = dw.Bits()
    for k in range(1000):
        b.put(k & 0x7f, 7)
    one = b.bytes()
    v = int.from_bytes(one, "little")
    assert all((v >> (7 * k)) & 0x7f == k & 0x7f for k in range(1000)) and len(one) == 875


def test_canonical_codes_are_the_rfcs():
    # RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) give 010 011 100 101 110 00 1110 1111
    want = [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]
    lens = [3, 3, 3, 3, 3, 2, 4, 4]
    got = dw.canonical_codes(lens)
    assert [(dw._reverse(c, n), n) for c, n in got] == list(zip(want, lens))
    fixed = dw.canonical_codes(dw.FIXED_LL)
    assert dw._reverse(fixed[0][0], 8) == 0b00110000 and dw._reverse(fixed[256][0], 7) == 0 and dw._reverse(fixed[280][0], 8) == 0b11000000


def test_kraft_complete_and_limited_lengths():
    rng = np.random.default_rng(1)
    for trial in range(300):
        n = int(rng.integers(2, 287))
        lens = dw.kraft_complete(n, rng=rng)
        assert len(lens) == n and max(lens) <= 15 and dw.is_complete(lens)
    lens = dw.kraft_complete(286, list(range(1, 14)) + [15] * 4, symbols=list(range(100, 117)))
    assert lens[100] == 1 and lens[116] == 15 and sum(1 for x in lens if x) == 17
    with pytest.raises(AssertionError):
        dw.kraft_complete(10, [1, 2])
    for trial in range(300):
        n = int(rng.integers(1, 287))
        freq = [int(f) for f in (rng.integers(0, 3, n) * rng.integers(1, 1 << int(rng.integers(1, 30)), n))]
        limit = int(rng.choice([7, 9, 15]))
        if sum(1 for f in freq if f) > 1 << limit or n < 2:
            continue
        lens = dw.limited_lengths(freq, limit)
        assert max(lens) <= limit and dw.is_complete(lens, limit)
        assert all(lens[s] for s, f in enumerate(freq) if f)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])    # a plain Huffman tree would be 39 deep
    lens = dw.limited_lengths(fib, 15)
    assert max(lens) == 15 and dw.is_complete(lens) and all(lens)


def test_symbols_of_lengths_and_distances():
    for n in range(3, 259):
        s = dw._LEN_SYM[n] - 257
        assert dw.LEN_BASE[s] <= n < dw.LEN_BASE[s] + (1 << dw.LEN_EXTRA[s]) and (s == 28) == (n == 258)
    for d in range(1, 32769):
        s = dw.dist_symbol(d)
        assert dw.DIST_BASE[s] <= d < dw.DIST_BASE[s] + (1 << dw.DIST_EXTRA[s])


def test_expand_and_every_block_type_round_trip():
    tokens = list(b"abcde") + [(3, 5), (10, 1), (258, 2), 120, (4, 18, ), (258, 7, 284)]
    want = bytearray(b"abcde")
    for n, d in ((3, 5), (10, 1), (258, 2)):
        for _ in range(n):
            want.append(want[-d])
    want.append(120)
    for n, d in ((4, 18), (258, 7)):
        for _ in range(n):
            want.append(want[-d])
    assert dw.expand(tokens) == bytes(want)
    assert dw.expand([(3, 2)], history=b"xy") == b"xyx"
    with pytest.raises(AssertionError):
        dw.expand([65, (3, 2)])
    for runs in (False, True):
        b = dw.Bits()
        dw.stored_block(b, b"stored", False)
        dw.fixed_block(b, tokens, False)
        dw.dynamic_block(b, tokens, False, runs=runs)
        dw.dynamic_block(b, tokens, True, runs=runs, hclen=19)
        d = zlib.decompressobj(-15)
        out = d.decompress(b.bytes())
        assert d.eof and out == b"stored" + dw.expand(tokens + tokens + tokens, history=b"stored")[0:]


def test_rle_lengths_say_the_same_lengths():
    rng = np.random.default_rng(2)
    for trial in range(200):
        seq = []
        while len(seq) < 316:
            seq += [int(rng.integers(0, 16)) if rng.random() < 0.7 else 0] * int(rng.choice([1, 2, 3, 6, 7, 10, 11, 12, 138, 139, 150]))
        seq = seq[:316]
        back = []
        for s, x in dw.rle_lengths(seq):
            if s < 16:
                back.append(s)
            elif s == 16:
                assert 0 <= x < 4 and back
                back += [back[-1]] * (3 + x)
            elif s == 17:
                assert 0 <= x < 8
                back += [0] * (3 + x)
            else:
                assert 0 <= x < 128
                back += [0] * (11 + x)
        assert back == seq


def test_bgzf_member():
    import gzip
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = b"member " * 100
    payload = co.compress(data) + co.flush()
    m = dw.bgzf_member(payload, len(data), zlib.crc32(data))
    assert len(m) == 18 + len(payload) + 8 and m[16] | m[17] << 8 == len(m) - 1
    assert gzip.decompress(m) == data
    dw.bgzf_member(bytes(dw.MAX_PAYLOAD), 0)
    with pytest.raises(AssertionError):
        dw.bgzf_member(bytes(dw.MAX_PAYLOAD + 1), 0)
