"""The corpus of hand-made DEFLATE streams for both inflaters (bgzf_decode + bgzf_resolve on the device, fastInflate on
the host): legal streams that zlib's own encoder never writes, and malformed ones.  Built with tests/deflate_writer.py.

build() returns Case(name, payload, isize, expected): the raw DEFLATE payload of one BGZF member, the ISIZE that goes
with it, and the bytes it must inflate to (deflate_writer.expand of the tokens) -- or None: must be refused.  Names
are "<group>/<case>"; the groups "refuse" (zlib is the judge) and "refuse-isize" (the project's own contract: the
stream must yield exactly ISIZE bytes) hold the malformed ones.  tests/test_deflate_writer.py holds every case against
zlib, so that a mistake here cannot pass as a decoder's."""
import collections
import functools
import time

import numpy as np

from deflate_writer import (DIST_BASE, DIST_EXTRA, EOB, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, MAX_PAYLOAD, Bits,
                            canonical_codes, dynamic_block, dynamic_header, expand, fixed_block, kraft_complete,
                            limited_lengths, put_tokens, stored_block, token_frequencies)

Case = collections.namedtuple("Case", "name payload isize expected")

N_FUZZ = 200
WINDOW = 1024  # output positions bgzf_resolve takes at a time
BATCH = 64     # matches it deals out at a time, in output order


class _Stream:
    """The blocks of one member and the tokens they hold, in order."""

    def __init__(self):
        self.b, self.tokens, self.starts = Bits(), [], []

    def _start(self, kind):
        self.starts.append((kind, self.b.bit_length % 8))

    def stored(self, data, final=False):
        self._start("stored")
        stored_block(self.b, bytes(data), final)
        self.tokens += list(data)

    def fixed(self, tokens, final=False):
        self._start("fixed")
        fixed_block(self.b, tokens, final)
        self.tokens += tokens

    def dynamic(self, tokens, final=False, **kw):
        self._start("dynamic")
        dynamic_block(self.b, tokens, final, **kw)
        self.tokens += tokens

    def case(self, name, trailing=b""):
        out = expand(self.tokens)
        payload = self.b.bytes() + trailing
        assert len(payload) <= MAX_PAYLOAD and len(out) <= 65536, (name, len(payload), len(out))
        return Case(name, payload, len(out), out)


class _Script:
    """Tokens by output position: random literals from a small alphabet up to a position, then a match there."""

    def __init__(self, seed, alphabet=16):
        self.rng, self.alphabet, self.t, self.pos = np.random.default_rng(seed), alphabet, [], 0

    def lits(self, n):
        self.t += [int(v) + 65 for v in self.rng.integers(0, self.alphabet, n)]
        self.pos += n

    def lit_to(self, pos):
        assert pos >= self.pos
        self.lits(pos - self.pos)

    def match(self, length, dist, sym=None):
        assert 1 <= dist <= self.pos
        self.t.append((length, dist) if sym is None else (length, dist, sym))
        self.pos += length

    def case(self, name):
        s = _Stream()
        s.dynamic(self.t, True)
        return s.case(name)


def _trim(lens, least):
    lens = list(lens)
    while len(lens) > least and lens[-1] == 0:
        lens.pop()
    return lens


# ------------------------------------------------------------------------------------------------ code shapes
def _flat286():
    ll = [8] * 226 + [9] * 60
    dl = [4] * 2 + [5] * 28
    t = [k & 255 for k in range(129 * 256)]  # every literal; 33 024 bytes, so that every distance is in reach
    for s in range(29):                      # every length symbol, with its smallest and largest extra bits
        hi = LEN_BASE[s] + (1 << LEN_EXTRA[s]) - 1
        t += [(LEN_BASE[s], 1 + 7 * s), 7, (hi, 300 + s, 257 + s), 9]
    for s in range(30):                      # every distance symbol, likewise
        t += [(3 + s, DIST_BASE[s]), 11, (4, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1), 13]
    s = _Stream()
    s.dynamic(t, True, ll_lens=ll, d_lens=dl)
    fl, fd = token_frequencies(t)
    assert all(fl) and all(fd)
    return [s.case("shape/flat286")]


DEPTH15 = list(range(1, 14)) + [15] * 4


def _depth15_codes():
    """Literal/length: 15 bits for literals 0xAA and 0x55, for 257 (length 3, no extra bits) and for 284 (5 extra bits);
    1 .. 13 bits for what builds the prefix and for the other lengths of 131 and more.  Distance: the same shape, 29 deep."""
    ll_syms = [0x41, 285, EOB, 0x42, 0x43, 283, 282, 281, 0x44, 0x45, 0x46, 0x47, 0x48] + [0xAA, 0x55, 257, 284]
    d_syms = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12] + [26, 27, 28, 29]
    ll = kraft_complete(286, DEPTH15, symbols=ll_syms)
    dl = kraft_complete(30, DEPTH15, symbols=d_syms)
    assert ll[0xAA] == ll[0x55] == ll[257] == ll[284] == 15 and dl[29] == 15
    return ll, dl


def _depth15():
    ll, dl = _depth15_codes()
    prefix = [0x41] + [(258, 1)] * 96  # 24 769 bytes from codes of 1 and 2 bits
    base = 1 + 96 * 258
    cases = []
    # (a) two 15-bit literals and a 15 + 15 + 13-bit match of length 3: 73 bits a trip, 7 000 trips
    t, pos = list(prefix), base
    for k in range(7000):
        pos += 2
        t += [0xAA, 0x55, (3, 24577 + (k * 2731) % min(8192, pos - 24576), 257)]
        pos += 3
    s = _Stream()
    s.dynamic(t, True, ll_lens=ll, d_lens=dl)
    cases.append(s.case("shape/depth15-a"))
    # (b) the same with lengths 131 .. 258: 284 takes 15 + 5 bits (78 bits a trip, 258 as 284 + 31), 281 .. 283 fewer.
    # 65 536 bytes of output hold about 180 such trips, so three members carry them.
    for half in range(3):
        t, pos, trips = list(prefix), base, 0
        while True:
            k = 3 * trips + half
            length = 258 if k % 5 == 0 else 227 + (k * 7) % 31 if k % 5 < 3 else 131 + (k * 11) % 96
            if pos + 2 + length > 65536:
                break
            pos += 2
            t += [0x55, 0xAA, (length, 24577 + (k * 5417) % min(8192, pos - 24576)) + ((284,) if length == 258 else ())]
            pos += length
            trips += 1
        assert trips >= 180
        s = _Stream()
        s.dynamic(t, True, ll_lens=ll, d_lens=dl)
        cases.append(s.case(f"shape/depth15-b{half}"))
    return cases


def _few_codes():
    cases = []
    sc = _Script(21)
    sc.lits(40)
    for k in range(60):
        sc.match(3 + (k * 17) % 256, 1)
        sc.lits(1 + k % 3)
    fl, _ = token_frequencies(sc.t)
    s = _Stream()
    s.dynamic(sc.t, True, ll_lens=_trim(limited_lengths(fl), 257), d_lens=[1])   # HDIST = 1: one code of one bit
    cases.append(s.case("shape/one-distance-code"))
    sc = _Script(22)
    sc.lits(500)
    s = _Stream()
    s.dynamic(sc.t, True, d_lens=[0])
    cases.append(s.case("shape/no-distance-code"))
    eob_only = dict(ll_lens=[0] * 256 + [1], d_lens=[0])
    s = _Stream()
    s.dynamic([], True, **eob_only)
    cases.append(s.case("shape/eob-only"))
    assert cases[-1].isize == 0
    s = _Stream()
    s.fixed(list(b"before"))
    s.dynamic([], False, **eob_only)
    s.stored(b"between")
    s.dynamic([], False, **eob_only)
    s.dynamic([], False, **eob_only)
    s.fixed(list(b"after") + [(6, 18)], True)
    cases.append(s.case("shape/eob-only-between"))
    return cases


def _tokens(seed, literals, lengths, dists, n_matches=40, lead=400):
    """`lead` literals, then matches with a literal or two between them; lengths and distances drawn from what has a code."""
    rng = np.random.default_rng(seed)
    t = [literals[int(i)] for i in rng.integers(0, len(literals), lead)]
    for _ in range(n_matches):
        t.append((lengths[int(rng.integers(0, len(lengths)))], dists[int(rng.integers(0, len(dists)))]))
        t += [literals[int(i)] for i in rng.integers(0, len(literals), int(rng.integers(0, 3)))]
    return t


def _run_crosses(syms, sym, nlit):
    at = 0
    for s, x in syms:
        n = {16: 3 + x, 17: 3 + x, 18: 11 + x}.get(s, 1)
        if s == sym and at < nlit < at + n:
            return True
        at += n
    return False


def _header_runs():
    cases = []

    def add(name, t, ll, dl, **kw):
        b = Bits()
        syms = dynamic_header(b, True, ll, dl, **kw)
        put_tokens(b, t, ll, dl)
        out = expand(t)
        cases.append(Case(name, b.bytes(), len(out), out))
        return syms

    lits6 = list(range(65, 124))
    # 60 codes of 6 bits (59 literals and end-of-block) and 32 of 9 bits: complete
    # -- a 16 that repeats the last literal/length length into the distance lengths: 257 .. 285 and distances 0 .. 7 are all 9 bits long
    ll = kraft_complete(286, [6] * 60 + [9] * 32, symbols=lits6 + [EOB] + [200, 201, 202] + list(range(257, 286)))
    dl = [9] * 8 + [1, 2, 3, 4, 5, 6]
    t = _tokens(31, lits6 + [200, 201, 202], list(range(3, 259)), list(range(1, 129)))
    syms = add("header/16-across-boundary", t, ll, dl)
    assert _run_crosses(syms, 16, 286)
    # -- an 18 whose zeros end the literal/length lengths (270 .. 285) and begin the distance lengths (0 .. 9)
    ll = kraft_complete(286, [6] * 60 + [9] * 32, symbols=lits6 + [EOB] + list(range(200, 219)) + list(range(257, 270)))
    dl = [0] * 10 + [1, 2, 3, 4, 5, 6, 6]
    t = _tokens(32, lits6 + list(range(200, 219)), list(range(3, 23)), list(range(33, 385)))
    syms = add("header/18-across-boundary", t, ll, dl)
    assert _run_crosses(syms, 18, 286)
    # -- the same lengths without any run symbol
    syms = add("header/no-runs", t, ll, dl, runs=False)
    assert all(s < 16 for s, _ in syms)
    # -- HCLEN = 5, the fewest that can describe a block: 16, 17, 18, 0 and 8 (with HCLEN = 4 every length is 0 and the
    # end-of-block code is missing: refuse/hclen-4).  Literals 1 .. 255 and end-of-block, 8 bits each.
    ll = [0] + [8] * 256
    t = [1 + (k * 7) % 255 for k in range(600)]
    b = Bits()
    dynamic_header(b, True, ll, [0])
    assert (int.from_bytes(b.bytes()[:3], "little") >> 13) & 15 == 1, "HCLEN = 5"
    add("header/hclen-5", t, ll, [0])
    # -- HCLEN = 19 with nothing behind the fifth length, and with symbol 15 (the last in the order) in use
    add("header/hclen-19", t, ll, [0], hclen=19)
    ll15, dl15 = _depth15_codes()
    add("header/hclen-19-used", [0x41, 0xAA, (258, 1), 0x55, (3, 2, 257)], ll15, dl15, runs=False)
    # -- a code-length code of depth 7: 1, 2, ..., 6, 7, 7 bits
    cl = [0] * 19
    for s, n in {0: 1, 6: 2, 9: 3, 16: 4, 18: 5, 17: 6, 1: 7, 2: 7}.items():
        cl[s] = n
    ll = kraft_complete(286, [6] * 60 + [9] * 32, symbols=lits6 + [EOB] + [200, 201, 202] + list(range(257, 286)))
    t = _tokens(33, lits6 + [200, 201, 202], list(range(3, 259)), [1, 2, 3])
    syms = add("header/code-length-code-depth-7", t, ll, [1, 2, 2], cl_lens=cl)
    assert {s for s, _ in syms} >= {6, 9, 1, 2, 16, 18}  # (1 and 2: the 7-bit codes)
    return cases


# ------------------------------------------------------------------------------------------------ block structure
def _block_structure():
    cases = []
    text = list(b"The quick brown fox jumps over the lazy dog. " * 6)
    # 300 empty fixed blocks, 10 bits each: their headers start at bit 0, 2, 4, 6; with one 19-bit block first at 1, 3, 5, 7
    for odd in (False, True):
        s = _Stream()
        if odd:
            s.fixed([200])  # 3 + 9 + 7 bits
        for _ in range(300):
            s.fixed([])
        s.fixed(text, True)
        assert {p for k, p in s.starts[-300:]} == ({1, 3, 5, 7} if odd else {0, 2, 4, 6})
        cases.append(s.case("blocks/300-empty-fixed" + ("-odd" if odd else "")))
    # every block type starting at every bit phase: fixed blocks of 10 and 19 bits move the phase to where it is wanted
    s = _Stream()
    for kind in ("stored", "fixed", "dynamic"):
        for phase in range(8):
            while s.b.bit_length % 8 != phase:
                s.fixed([200] if (phase - s.b.bit_length) % 2 else [])
            if kind == "stored":
                s.stored(b"" if phase % 2 else bytes([phase] * 3))
            elif kind == "fixed":
                s.fixed([] if phase % 2 else [66, 200, (3, 2)])
            else:
                s.dynamic([67 + phase, 68, 67 + phase, (4, 3)] if phase % 3 else [])
    s.fixed(text, True)
    assert {(k, p) for k, p in s.starts} >= {(k, p) for k in ("stored", "fixed", "dynamic") for p in range(8)}
    cases.append(s.case("blocks/every-type-at-every-phase"))
    # the largest stored block that fits a member
    rng = np.random.default_rng(41)
    s = _Stream()
    s.stored(rng.integers(0, 256, MAX_PAYLOAD - 5, dtype=np.uint8).tobytes(), True)
    assert len(s.b.bytes()) == MAX_PAYLOAD
    cases.append(s.case("blocks/largest-stored"))
    # later blocks' matches read what a stored block wrote
    s = _Stream()
    s.stored(rng.integers(0, 256, 1000, dtype=np.uint8).tobytes())
    s.fixed([(258, 1000), 1, (3, 1), (100, 700), 2, (50, 1200)])
    s.dynamic([3, (258, 1400), (30, 1000), 4, 5, (200, 1700), (9, 8)])
    s.stored(rng.integers(0, 256, 77, dtype=np.uint8).tobytes())
    s.dynamic([(77, 77), (258, 2000), 6], True)
    cases.append(s.case("blocks/stored-as-match-source"))
    # 9 bytes behind the final block, inside the payload
    s = _Stream()
    s.dynamic(text + [(40, 45), (258, 1)], True)
    cases.append(s.case("blocks/trailing-bytes", trailing=b"\xff\x00\xa5trailing"[:9]))
    return cases


# ------------------------------------------------------------------------------------------------ match geometry
def _all_pairs():
    """Every (distance 1 .. 40, length 3 .. 258), each behind two to four fresh literals, in a seeded order."""
    rng = np.random.default_rng(51)
    pairs = [(n, d) for d in range(1, 41) for n in range(3, 259)]
    order = rng.permutation(len(pairs))
    cases, t, pos, seen = [], None, 0, set()

    def close():
        s = _Stream()
        s.dynamic(t, True)
        seen.update(tok for tok in t if isinstance(tok, tuple))
        cases.append(s.case(f"pairs/{len(cases):02d}"))

    for i in order:
        n, d = pairs[int(i)]
        if t is None or pos + 4 + n > 65536:
            if t is not None:
                close()
            t = [int(v) for v in rng.integers(0, 256, 40)]
            pos = 40
        k = int(rng.integers(2, 5))
        t += [int(v) for v in rng.integers(0, 256, k)] + [(n, d)]
        pos += k + n
    close()
    assert seen == set(pairs) and len(seen) == 40 * 256
    return cases


def _chains():
    cases = []
    for n, d in ((3, 3), (4, 4), (3, 6), (258, 258), (3, 1)):
        sc = _Script(60 + n + d, alphabet=26)
        sc.lits(d)
        while sc.pos + n <= 65536:
            sc.match(n, d)
        sc.lit_to(65536)
        cases.append(sc.case(f"chains/len{n}-dist{d}"))
        assert cases[-1].isize == 65536
    return cases


def _spans():
    sc = _Script(71)
    # a source in the previous window of 1 024 positions, covering matches there
    sc.lit_to(WINDOW + 76)
    for _ in range(20):
        sc.match(5, 7)
        sc.lits(1)
    sc.lit_to(2 * WINDOW + 10)
    sc.match(60, sc.pos - (WINDOW + 70))
    # a source over several earlier matches and literals of the same batch
    sc.lit_to(3 * WINDOW + 8)
    for _ in range(10):
        sc.match(3, 9)
        sc.lits(2)
    sc.match(40, 45)
    sc.match(90, 30)  # ... and one that overlaps itself on top of them
    # a source that starts inside one earlier match and ends inside another
    sc.lit_to(4 * WINDOW + 4)
    a = sc.pos
    sc.match(20, 30)
    sc.lits(5)
    sc.match(20, 40)
    sc.lits(3)
    sc.match(30, sc.pos - (a + 10))
    # more than 64 matches in one window: a source in the previous batch, and one across the two batches
    sc.lit_to(5 * WINDOW)
    a = sc.pos
    for _ in range(BATCH + 6):
        sc.match(3, 11)
    sc.match(100, sc.pos - (a + 5))
    sc.match(40, sc.pos - (a + 3 * BATCH - 20))
    sc.match(50, 4)
    # a chain through a whole batch: every match reads the end of the one before
    sc.lit_to(6 * WINDOW + 1)
    for k in range(2 * BATCH):
        sc.match(4 + k % 3, 2 + k % 5)
    sc.lits(7)
    return [sc.case("spans/sources-across-matches-batches-windows")]


def _edges():
    cases = []
    for name, starts in (("edges/starts-63-1023-65533", (63, 1023, 65533)), ("edges/starts-64-1024", (64, 1024))):
        sc = _Script(81)
        for p in starts:
            sc.lit_to(p)
            sc.match(3 if p == 65533 else 5, 10)
        sc.lit_to(65536)
        cases.append(sc.case(name))
    sc = _Script(82)
    sc.lit_to(997)
    sc.match(3, 500)
    cases.append(sc.case("edges/match-at-isize-minus-3"))
    assert cases[-1].isize == 1000
    sc = _Script(83)
    sc.lit_to(1000)
    sc.match(100, 50)     # over the 1 024 boundary, overlapping
    sc.lit_to(2040)
    sc.match(20, 1500)    # over the next one, not overlapping
    sc.lits(3)
    cases.append(sc.case("edges/match-across-1024"))
    sc = _Script(84)
    sc.lits(1)
    sc.match(258, 1)      # dist == pos at 1
    sc.lit_to(300)
    sc.match(30, 300)     # dist == pos, no overlap
    sc.match(258, 330)    # dist == pos, reading the match before
    sc.lits(2)
    cases.append(sc.case("edges/distance-equals-position"))
    for sym in (285, 284):
        sc = _Script(85)
        sc.lit_to(32768)
        sc.match(10, 32768)   # the first byte of the block, from as far as a distance reaches
        sc.match(3, 32768)
        sc.lits(4)
        sc.match(258, 100, sym)
        sc.lit_to(65536 - 258)
        sc.match(258, 32768, sym)
        assert sc.pos == 65536
        cases.append(sc.case(f"edges/far-matches-258-as-{sym}"))
    sc = _Script(86)      # literals only for thousands of positions: bitmap words that are never written
    sc.lits(5)
    sc.match(4, 5)
    sc.lits(5000)
    sc.match(3, 4000)
    sc.lits(20000)
    sc.match(258, 25000)
    sc.lits(9000)
    sc.match(7, 1)
    cases.append(sc.case("edges/long-literal-stretches"))
    return cases


# ------------------------------------------------------------------------------------------------ token fuzz
def _fuzz_member(seed):
    rng = np.random.default_rng(seed)
    target = int(rng.integers(1, 8193))
    alphabet = int(rng.choice([2, 4, 20, 256]))
    p_match = float(rng.choice([0.1, 0.5, 0.9]))
    t, pos = [], 0
    while pos < target:
        if pos == 0 or rng.random() >= p_match:
            t.append(int(rng.integers(0, alphabet)) if alphabet < 256 else int(rng.integers(0, 256)))
            pos += 1
            continue
        n = int(rng.integers(3, 259)) if rng.random() < 0.5 else int(rng.integers(3, 12))
        n = min(n, target - pos)
        if n < 3:
            t.append(int(rng.integers(0, alphabet)))
            pos += 1
            continue
        d = int(rng.integers(1, pos + 1)) if rng.random() < 0.5 else int(rng.integers(1, min(pos, 40) + 1))
        t.append((n, d, 284) if n == 258 and rng.random() < 0.5 else (n, d))
        pos += n
    out = expand(t)
    # the tokens in 1 .. 20 blocks of random types
    cuts = sorted({int(c) for c in rng.integers(1, len(t), int(rng.integers(0, 20)))} - {0, len(t)}) if len(t) > 1 else []
    s, at, edges = _Stream(), 0, [0] + cuts + [len(t)]
    for k in range(len(edges) - 1):
        part, final = t[edges[k]:edges[k + 1]], k == len(edges) - 2
        n_out = sum(x[0] if isinstance(x, tuple) else 1 for x in part)
        kind = int(rng.integers(0, 4))
        if kind == 0:
            stored_block(s.b, out[at:at + n_out], final)
        elif kind == 1:
            fixed_block(s.b, part, final)
        elif kind == 2:
            dynamic_block(s.b, part, final, runs=bool(rng.integers(0, 2)), hclen=[None, 19][int(rng.integers(0, 2))])
        else:  # random complete codes over the symbols in use and a few more
            fl, fd = token_frequencies(part)
            ul = [i for i, f in enumerate(fl) if f]
            ul += [int(x) for x in rng.permutation([i for i in range(286) if not fl[i]])[:int(rng.integers(1, 30))]]
            ud = [i for i, f in enumerate(fd) if f]
            ud += [int(x) for x in rng.permutation([i for i in range(30) if not fd[i]])[:int(rng.integers(2 - min(len(ud), 1), 6))]]
            ll = _trim(kraft_complete(286, symbols=ul, rng=rng), 257)
            dl = _trim(kraft_complete(30, symbols=ud, rng=rng), 1)
            dynamic_block(s.b, part, final, ll_lens=ll, d_lens=dl, runs=bool(rng.integers(0, 2)))
        at += n_out
    payload = s.b.bytes()
    assert at == len(out) and len(payload) <= MAX_PAYLOAD
    return Case(f"fuzz/{seed - 1000:03d}", payload, len(out), out)


# ------------------------------------------------------------------------------------------------ refused streams
def _refuse():
    cases = []

    def add(name, b, isize=64, pad=8):
        data = b if isinstance(b, bytes) else b.bytes() + bytes(pad)
        cases.append(Case("refuse/" + name, data, isize, None))

    lits = list(b"refuse me, please: 0123456789")
    b = Bits()
    b.put(1 | 3 << 1, 3)
    add("reserved-btype", b)
    b = Bits()
    b.put(1, 3)
    b.align()
    b.put(5 | (5 ^ 0xffff ^ 0x100) << 16, 32)
    b.raw_bytes(b"12345")
    add("len-nlen-mismatch", b, 5, pad=0)
    b = Bits()
    b.put(1, 3)
    b.align()
    b.put(100 | (100 ^ 0xffff) << 16, 32)
    b.raw_bytes(b"only ten..")
    add("stored-past-payload", b, 100, pad=0)
    # a good code in the first 286 / 30 lengths; only the counts are out of range
    ll, dl = limited_lengths(token_frequencies(lits + [(5, 3)])[0]), [1, 1]
    for n in (287, 288):
        b = Bits()
        dynamic_header(b, True, ll + [0] * (n - 286), dl)
        put_tokens(b, lits, ll, dl)
        add(f"hlit-{n}", b, len(lits))
    for n in (31, 32):
        b = Bits()
        dynamic_header(b, True, _trim(ll, 257), dl + [0] * (n - 2))
        put_tokens(b, lits, ll, dl)
        add(f"hdist-{n}", b, len(lits))
    ll = _trim(ll, 257)
    # the code-length symbols by hand
    good = [(n, 0) for n in ll + dl]
    b = Bits()
    dynamic_header(b, True, ll, dl, cl_syms=[(16, 0)] + good[3:])
    put_tokens(b, lits, ll, dl)
    add("16-first", b, len(lits))
    b = Bits()
    dynamic_header(b, True, ll, dl, cl_syms=good[:-2] + [(18, 0)])  # 11 zeros where 2 lengths are left
    put_tokens(b, lits, ll, dl)
    add("run-past-the-lengths", b, len(lits))
    b = Bits()
    dynamic_header(b, True, ll, dl, cl_syms=good[:-2] + [(16, 3)])  # 6 repeats where 2 lengths are left
    put_tokens(b, lits, ll, dl)
    add("repeat-past-the-lengths", b, len(lits))
    cl = [0] * 19
    for n in set(ll + dl):
        cl[n] = 3
    assert 2 <= sum(1 for n in cl if n) < 8
    b = Bits()
    dynamic_header(b, True, ll, dl, runs=False, cl_lens=cl)
    put_tokens(b, lits, ll, dl)
    add("incomplete-code-length-code", b, len(lits))
    cl = [0] * 19
    cl[0] = cl[18] = 1
    b = Bits()
    dynamic_header(b, True, [0] * 257, [0], cl_lens=cl, hclen=4)       # all that HCLEN = 4 can say: every length is 0
    add("hclen-4", b, 0)
    for name, code in (("over-subscribed-literal-set", {65: 1, 66: 1, EOB: 1}), ("incomplete-literal-set", {65: 2, EOB: 2}),
                       ("no-end-of-block-code", {65: 1, 66: 1})):
        l2 = [0] * 257
        for s, n in code.items():
            l2[s] = n
        b = Bits()
        dynamic_header(b, True, l2, [0])
        put_tokens(b, [65, 65, 65], l2, [0], eob=EOB in code and l2[EOB] > 0)
        add(name, b, 3)
    b = Bits()
    dynamic_header(b, True, ll, [2, 2])
    put_tokens(b, lits, ll, [2, 2])
    add("incomplete-distance-set", b, len(lits))
    # 286 and 30 have codes in the fixed block's sets and no meaning
    b = Bits()
    b.put(1 | 1 << 1, 3)
    put_tokens(b, lits + [286], FIXED_LL, FIXED_D)
    add("fixed-literal-length-286", b, len(lits))
    b = Bits()
    b.put(1 | 1 << 1, 3)
    put_tokens(b, lits, FIXED_LL, FIXED_D, eob=False)
    c, n = canonical_codes(FIXED_LL)[257]
    b.put(c, n)
    c, n = canonical_codes(FIXED_D)[30]
    b.put(c, n)
    put_tokens(b, [], FIXED_LL, FIXED_D)
    add("fixed-distance-30", b, len(lits) + 3)
    # a one-code distance set: '0' is distance 1, '1' is nothing
    b = Bits()
    dynamic_header(b, True, ll, [1])
    put_tokens(b, lits, ll, [1], eob=False)
    c, n = canonical_codes(ll)[259]
    b.put(c, n)
    b.put(1, 1)
    put_tokens(b, [], ll, [1])
    add("unused-code-of-one-distance-code", b, len(lits) + 5)
    b = Bits()
    dynamic_header(b, True, ll, [0])
    put_tokens(b, lits, ll, [0], eob=False)
    b.put(c, n)
    b.put(0, 1)
    put_tokens(b, [], ll, [0])
    add("length-without-distance-codes", b, len(lits) + 5)
    # distances that reach before the block's first byte
    b = Bits()
    fixed_block(b, lits + [(4, len(lits) + 1)], True)
    add("distance-past-start", b, len(lits) + 4)
    b = Bits()
    dynamic_block(b, lits + [(200, len(lits) + 1)] + lits, True)
    add("distance-past-start-dynamic", b, 2 * len(lits) + 200)
    b = Bits()
    fixed_block(b, [(3, 1)] + lits, True)
    add("match-first", b, len(lits) + 3)
    b = Bits()
    stored_block(b, b"stored", False)
    fixed_block(b, [(3, 7)], True)
    add("distance-past-start-after-stored", b, 9)
    # cut inside a code: the last whole byte holds the start of a 15-bit literal
    ll15, dl15 = _depth15_codes()
    b = Bits()
    dynamic_header(b, True, ll15, dl15)
    put_tokens(b, [0x41] * 5 + [0xAA] * 40, ll15, dl15)
    data = b.bytes()
    add("truncated-mid-code", data[:-8], 45)
    return cases


def _refuse_isize():
    """Streams that zlib takes, with an ISIZE they do not yield."""
    cases = []
    lits = list(b"exactly as many bytes as ISIZE says")

    def add(name, s, isize):
        cases.append(Case("refuse-isize/" + name, s.b.bytes(), isize, None))

    s = _Stream()
    s.dynamic(lits + [(20, 5)], True)
    add("match-past-isize", s, len(lits) + 7)
    s = _Stream()
    s.dynamic(lits + [(3, 5)], True)
    add("3-byte-match-past-isize", s, len(lits) + 2)
    s = _Stream()
    s.dynamic(lits + lits, True)
    add("literal-past-isize", s, len(lits) + 1)
    s = _Stream()
    s.fixed(lits + [(20, 5)], True)
    add("stream-one-short-of-isize", s, len(lits) + 21)
    s = _Stream()
    s.fixed(lits)
    s.stored(b"stored tail", True)
    add("isize-one-short-of-stream", s, len(lits) + 10)
    return cases


GROUPS = ("shape", "header", "blocks", "pairs", "chains", "spans", "edges", "fuzz", "refuse", "refuse-isize")


@functools.lru_cache(maxsize=None)
def build():
    """All cases, built once per process: (cases, seconds it took)."""
    t0 = time.perf_counter()
    cases = _flat286() + _depth15() + _few_codes() + _header_runs() + _block_structure()
    cases += _all_pairs() + _chains() + _spans() + _edges()
    fuzz = [_fuzz_member(1000 + k) for k in range(N_FUZZ)]
    assert len(fuzz) == N_FUZZ
    cases += fuzz + _refuse() + _refuse_isize()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) and all(n.split("/")[0] in GROUPS for n in names)
    for c in cases:
        assert len(c.payload) <= MAX_PAYLOAD and c.isize <= 65536, c.name
    return tuple(cases), time.perf_counter() - t0


def accept_cases():
    return [c for c in build()[0] if c.expected is not None]


def refuse_cases():
    return [c for c in build()[0] if c.expected is None]


def corpus_records(cases):
    """The corpus as fast_inflate_check reads it: u32 in_len, u32 out_len, u8 accept, the payload."""
    import struct
    return b"".join(struct.pack("<IIB", len(c.payload), c.isize, c.expected is not None) + c.payload for c in cases)
