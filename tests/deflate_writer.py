"""A token-level DEFLATE writer (RFC 1951) and its own reference, for streams that no encoder at hand produces.

The writer emits exactly the tokens, codes and header encoding it is given -- legal choices that zlib's encoder never
makes (15-bit codes, a one-code distance set, length 258 as symbol 284 + 31, chains of overlapping 3-byte matches, ...) and,
through `Bits.put`, any malformed header.  `expand` is the expected output: plain LZ77 expansion of the same tokens, neither
zlib nor one of the decoders under test.  tests/test_deflate_writer.py holds the writer itself against zlib.

Tokens: an int 0..255 is a literal; a tuple (length, distance) or (length, distance, length_symbol) is a match, the third
member forcing the length symbol (284 for length 258)."""
import heapq
import struct

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
EOB = 256
MAX_PAYLOAD = 65510  # BSIZE is 16 bits: 65536 - 18 header bytes - 8 footer bytes

FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def _length_symbol(length):
    if length == 258:
        return 285
    s = 28
    while LEN_BASE[s] > length:
        s -= 1
    return 257 + s


_LEN_SYM = [0, 0, 0] + [_length_symbol(n) for n in range(3, 259)]


def dist_symbol(dist):
    s = 29
    while DIST_BASE[s] > dist:
        s -= 1
    return s


def _reverse(code, nbits):
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


class Bits:
    """LSB-first bit packing of a DEFLATE stream; Huffman codes go in MSB-first (`code`), everything else as it is (`put`)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 512:
            whole = self.n >> 3
            self.out += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
            self.acc >>= 8 * whole
            self.n -= 8 * whole

    def code(self, code, nbits):
        self.put(_reverse(code, nbits), nbits)

    @property
    def bit_length(self):
        return 8 * len(self.out) + self.n

    def align(self):
        self.put(0, -self.bit_length % 8)

    def raw_bytes(self, data):
        """Whole bytes at a byte boundary (the body of a stored block)."""
        assert self.bit_length % 8 == 0
        self.out += (self.acc & ((1 << self.n) - 1)).to_bytes(self.n >> 3, "little")
        self.acc, self.n = 0, 0
        self.out += data

    def bytes(self):
        nbytes = (self.n + 7) >> 3
        return bytes(self.out) + (self.acc & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little")


def canonical_codes(lens):
    """RFC 1951 3.2.2: [(code bit-reversed for one `put`, length)] per symbol; (0, 0) for an unused one.  The lengths are
    taken as they are (an over-subscribed or incomplete set gives the codes the RFC's algorithm gives)."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lens:
        if n == 0:
            out.append((0, 0))
        else:
            out.append((_reverse(nxt[n] & ((1 << n) - 1), n), n))
            nxt[n] += 1
    return out


def kraft_sum(lens, limit=15):
    return sum(1 << (limit - n) for n in lens if n)


def is_complete(lens, limit=15):
    return kraft_sum(lens, limit) == 1 << limit


def random_depths(k, rng, limit=15):
    """The leaf depths of a random full binary tree with k >= 2 leaves, none deeper than `limit`."""
    assert 2 <= k <= 1 << limit
    depths = [1, 1]
    while len(depths) < k:
        i = int(rng.integers(0, len(depths)))
        if depths[i] >= limit:  # a random leaf that may still split (one exists: k <= 2^limit)
            i = min(range(len(depths)), key=lambda j: depths[j])
        depths[i] += 1
        depths.append(depths[i])
    return depths


def kraft_complete(n_symbols, depths=None, rng=None, symbols=None, limit=15):
    """Code lengths of `n_symbols` symbols that form a complete prefix code no deeper than `limit`.
    depths: the code lengths to hand out (their Kraft sum must be 1); None: those of a random tree over len(symbols)
            leaves -- or, without `symbols`, over a random number of them.
    symbols: who gets a code (in this order, unless an rng shuffles the depths); None: the first len(depths) symbols, or
             with an rng a random choice."""
    if depths is None:
        k = len(symbols) if symbols is not None else int(rng.integers(2, n_symbols + 1))
        depths = random_depths(k, rng, limit)
    depths = list(depths)
    assert max(depths) <= limit and is_complete(depths, limit), "not a complete code"
    if symbols is None:
        symbols = list(range(len(depths))) if rng is None else [int(s) for s in rng.permutation(n_symbols)[:len(depths)]]
    assert len(symbols) == len(depths) <= n_symbols and len(set(symbols)) == len(symbols)
    if rng is not None:
        depths = [depths[int(i)] for i in rng.permutation(len(depths))]
    lens = [0] * n_symbols
    for s, d in zip(symbols, depths):
        lens[s] = d
    return lens


def limited_lengths(freq, limit=15):
    """Huffman code lengths for the symbols with freq > 0, no longer than `limit`, always a complete code: with fewer
    than two symbols in use the lowest unused ones get a code too."""
    used = [s for s, f in enumerate(freq) if f > 0]
    weight = {s: freq[s] for s in used}
    for s in range(len(freq)):
        if len(weight) >= 2:
            break
        weight.setdefault(s, 1)
    heap = [(w, s, (s,)) for s, w in weight.items()]
    heapq.heapify(heap)
    depth = dict.fromkeys(weight, 0)
    while len(heap) > 1:
        w1, t1, m1 = heapq.heappop(heap)
        w2, t2, m2 = heapq.heappop(heap)
        for s in m1 + m2:
            depth[s] += 1
        heapq.heappush(heap, (w1 + w2, min(t1, t2), m1 + m2))
    for s in depth:
        depth[s] = min(depth[s], limit)
    full = 1 << limit
    k = sum(1 << (limit - d) for d in depth.values())
    by_weight = sorted(depth, key=lambda s: (weight[s], s))
    while k > full:  # over-subscribed after the clamp: lengthen the rarest symbol that can still grow
        s = max((s for s in by_weight if depth[s] < limit), key=lambda s: depth[s])
        k -= 1 << (limit - depth[s] - 1)
        depth[s] += 1
    while k < full:  # room left: shorten the most frequent symbol whose gain fits
        s = next(s for s in reversed(by_weight) if (1 << (limit - depth[s])) <= full - k)
        k += 1 << (limit - depth[s])
        depth[s] -= 1
    lens = [0] * len(freq)
    for s, d in depth.items():
        lens[s] = d
    assert is_complete(lens, limit)
    return lens


def token_frequencies(tokens):
    ll, d = [0] * 286, [0] * 30
    ll[EOB] = 1
    for t in tokens:
        if isinstance(t, tuple):
            ll[t[2] if len(t) > 2 else _LEN_SYM[t[0]]] += 1
            d[dist_symbol(t[1])] += 1
        else:
            ll[t] += 1
    return ll, d


def put_tokens(bits, tokens, ll_lens, d_lens, eob=True):
    """The tokens in the codes that the lengths define; every symbol used must have a code."""
    ll, dc = canonical_codes(ll_lens), canonical_codes(d_lens)
    for t in tokens:
        if not isinstance(t, tuple):
            c, n = ll[t]
            assert n, f"literal {t} has no code"
            bits.put(c, n)
            continue
        length, dist = t[0], t[1]
        ls = t[2] if len(t) > 2 else _LEN_SYM[length]
        lx = length - LEN_BASE[ls - 257]
        assert 0 <= lx < 1 << LEN_EXTRA[ls - 257], f"length {length} is not symbol {ls}'s"
        ds = dist_symbol(dist)
        c, n = ll[ls]
        d, m = dc[ds]
        assert n and m, f"match {t} has no code"
        v = c | lx << n
        n += LEN_EXTRA[ls - 257]
        v |= d << n
        n += m
        v |= (dist - DIST_BASE[ds]) << n
        bits.put(v, n + DIST_EXTRA[ds])
    if eob:
        c, n = ll[EOB]
        assert n, "no end-of-block code"
        bits.put(c, n)


def stored_block(bits, data, final):
    assert len(data) <= 0xffff
    bits.put(int(final), 3)  # BFINAL, BTYPE 00
    bits.align()
    bits.put(len(data) | (len(data) ^ 0xffff) << 16, 32)
    bits.raw_bytes(data)


def fixed_block(bits, tokens, final, eob=True):
    bits.put(int(final) | 1 << 1, 3)
    put_tokens(bits, tokens, FIXED_LL, FIXED_D, eob)


def rle_lengths(seq, runs=True):
    """The code lengths of both alphabets, back to back, as code-length symbols [(symbol, extra value)].  With runs:
    greedy 18 / 17 for zeros and 16 for repeats -- over the whole sequence, so a run may cross from the literal/length
    lengths into the distance lengths, as RFC 1951 3.2.7 allows."""
    if not runs:
        return [(n, 0) for n in seq]
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                out.append((18, n - 11))
                run -= n
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                out.append((16, n - 3))
                run -= n
        out += [(v, 0)] * run
        i = j
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_header(bits, final, ll_lens, d_lens, runs=True, hclen=None, cl_lens=None, cl_syms=None):
    """BFINAL, BTYPE 10, HLIT, HDIST, HCLEN, the code-length code and the lengths of both alphabets.
    ll_lens / d_lens: 257..288 and 1..32 lengths (what the 5-bit fields can say, legal or not).
    runs:    False: one code-length symbol per length; True: rle_lengths.
    cl_syms: the code-length symbols to write instead, [(symbol, extra value)].
    hclen:   how many code-length code lengths to write (4..19); None: as few as the symbols in use need.
    cl_lens: the 19 lengths of the code-length code; None: a Huffman code for the symbols in use, at most 7 bits."""
    assert 257 <= len(ll_lens) <= 288 and 1 <= len(d_lens) <= 32
    syms = cl_syms if cl_syms is not None else rle_lengths(list(ll_lens) + list(d_lens), runs)
    if cl_lens is None:
        freq = [0] * 19
        for s, _ in syms:
            freq[s] += 1
        cl_lens = limited_lengths(freq, 7)
    need = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl_lens[s]])
    hclen = need if hclen is None else hclen
    assert 4 <= need <= hclen <= 19, "HCLEN leaves out a code-length symbol that has a code"
    bits.put(int(final) | 2 << 1, 3)
    bits.put(len(ll_lens) - 257 | (len(d_lens) - 1) << 5 | (hclen - 4) << 10, 14)
    for s in CL_ORDER[:hclen]:
        bits.put(cl_lens[s], 3)
    codes = canonical_codes(cl_lens)
    for s, x in syms:
        c, n = codes[s]
        assert n, f"code-length symbol {s} has no code"
        bits.put(c | x << n, n + _CL_EXTRA.get(s, 0))
    return syms


def dynamic_block(bits, tokens, final, ll_lens=None, d_lens=None, eob=True, **header):
    """A dynamic block with the given code lengths; without them: limited_lengths of the tokens' own frequencies (a
    block without a match then has one distance length, 0)."""
    if ll_lens is None:
        fl, fd = token_frequencies(tokens)
        ll_lens = limited_lengths(fl)
        while len(ll_lens) > 257 and ll_lens[-1] == 0:
            ll_lens.pop()
        if d_lens is None:
            d_lens = limited_lengths(fd) if any(fd) else [0]
            while len(d_lens) > 1 and d_lens[-1] == 0:
                d_lens.pop()
    dynamic_header(bits, final, ll_lens, d_lens, **header)
    put_tokens(bits, tokens, ll_lens, d_lens, eob)


def expand(tokens, history=b""):
    """What the tokens mean: literals as they come, (length, distance) copied byte by byte from `distance` back."""
    out = bytearray(history)
    for t in tokens:
        if not isinstance(t, tuple):
            out.append(t)
            continue
        length, dist = t[0], t[1]
        assert 3 <= length <= 258 and 1 <= dist <= min(32768, len(out)), f"token {t} at {len(out)}"
        at = len(out) - dist
        if dist >= length:
            out += out[at:at + length]
        else:
            for k in range(length):
                out.append(out[at + k])
    return bytes(out[len(history):])


def bgzf_member(payload, isize, crc=0):
    """A BGZF member around a raw DEFLATE payload: the standard 18-byte header (XLEN 6, the BC subfield), CRC32, ISIZE.
    Neither decoder here checks the CRC."""
    assert len(payload) <= MAX_PAYLOAD, f"{len(payload)} payload bytes do not fit a BGZF member"
    hdr = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0])
    return hdr + struct.pack("<H", len(hdr) + 2 + len(payload) + 8 - 1) + payload + struct.pack("<II", crc, isize)
