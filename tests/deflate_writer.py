"""A test-only DEFLATE bit writer (RFC 1951): stored, fixed and dynamic blocks from explicit token lists and explicit code lengths --
the streams zlib's compressor will not produce on request (a match at distance 32768, 15-bit codes, a single distance code, repeat
codes that run from the literal/length lengths into the distance lengths, 286 and 30 codes, length symbol 284 with extra 31) and the
ones no compressor produces (block type 3, a wrong NLEN, over-subscribed lengths, a distance in front of the first byte).
tests/test_inflate.py checks every valid stream made here against zlib.decompress before it is used: an expected value is zlib's.

A token is an int (a literal), (length, distance), or ("len284", distance): length 258 as symbol 284 with extra bits 31."""

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
# a complete code over all 19 code-length symbols: 13 codes of 4 bits and 6 of 5
CL_DEFAULT = [4] * 13 + [5] * 6


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        """n bits of value, the lowest first (RFC 1951 3.1.1: everything but Huffman codes)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code of n bits, the highest bit first"""
        for i in range(n - 1, -1, -1):
            self.bits(code >> i & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """symbol -> (code, length) of the canonical Huffman code (RFC 1951 3.2.2); no check that the lengths are a code"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def length_symbol(length):
    s = max(i for i in range(29) if LEN_BASE[i] <= length)
    return s, length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s]


def put_tokens(w, tokens, ll, d):
    """the tokens and the end-of-block code in the codes ll / d (symbol -> (code, length))"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*ll[t])
            continue
        if t[0] == "len284":
            w.code(*ll[257 + 27]); w.bits(31, 5)
        else:
            s, x = length_symbol(t[0])
            w.code(*ll[257 + s]); w.bits(x, LEN_EXTRA[s])
        s, x = dist_symbol(t[1])
        w.code(*d[s]); w.bits(x, DIST_EXTRA[s])
    w.code(*ll[256])


def stored(w, data, final, nlen=None):
    w.bits(1 if final else 0, 1); w.bits(0, 2); w.align()
    w.bits(len(data), 16); w.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.bits(b, 8)


def fixed(w, tokens, final):
    w.bits(1 if final else 0, 1); w.bits(1, 2)
    put_tokens(w, tokens, canonical(FIXED_LL), canonical(FIXED_D))


def run_length_ops(seq):
    """the code-length sequence as (symbol, extra value, first position, positions covered): a run of 3..6 equal lengths behind
    their first as 16, 3..10 zeros as 17, 11..138 zeros as 18 -- over the literal/length and distance lengths as one sequence"""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            ops.append((18, take - 11, i, take) if take >= 11 else (17, take - 3, i, take))
            i += take
        elif v != 0 and run >= 4:
            ops.append((v, 0, i, 1))
            take = min(run - 1, 6)
            ops.append((16, take - 3, i + 1, take))
            i += 1 + take
        else:
            ops.append((v, 0, i, 1))
            i += 1
    return ops


def dynamic(w, tokens, final, ll_lens, d_lens, cl_lens=None, ops=None):
    """a dynamic block whose header states exactly ll_lens (257..286 entries) and d_lens (1..30 entries); cl_lens: the 19 lengths of
    the code-length code (default: a complete code over all 19); ops: the header's code-length symbols as (symbol, extra value, ...)
    (default: run_length_ops of the two lists as one sequence).  -> the ops written"""
    cl_lens = list(CL_DEFAULT) if cl_lens is None else list(cl_lens)
    ops = run_length_ops(list(ll_lens) + list(d_lens)) if ops is None else ops
    w.bits(1 if final else 0, 1); w.bits(2, 2)
    w.bits(len(ll_lens) - 257, 5); w.bits(len(d_lens) - 1, 5); w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for op in ops:
        w.code(*cl[op[0]])
        if op[0] >= 16:
            w.bits(op[1], {16: 2, 17: 3, 18: 7}[op[0]])
    put_tokens(w, tokens, canonical(ll_lens), canonical(d_lens))
    return ops


def expand(tokens):
    """the bytes a token list stands for (what the test means to encode; zlib says what the stream holds)"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n = 258 if t[0] == "len284" else t[0]
            for _ in range(n):
                out.append(out[-t[1]])
    return bytes(out)
