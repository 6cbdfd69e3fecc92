"""An unaligned BAM file written with struct and zlib alone (SAM specification 4.1 BGZF, 4.2 the BAM records): the test input of the
BAM reader (longqc_amd/csrc/reader.cpp, bgzf.hpp, kernels_bam.hpp).  No htslib: what a test expects of a file is the list it wrote."""
import struct
import zlib

CODES = b"=ACMGRSVTWYHKDBN"
_NIB = {c: i for i, c in enumerate(CODES)}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def pack_seq(seq):
    """two bases per byte, the first in the high nibble"""
    n = [_NIB[c] for c in seq]
    if len(n) & 1:
        n.append(0)
    return bytes(n[i] << 4 | n[i + 1] for i in range(0, len(n), 2))


def record(name, seq, qual=None, cigar=(), tags=b"", flag=4):
    """one alignment record; qual: Phred values (bytes), None: 0xff throughout (no qualities)"""
    q = b"\xff" * len(seq) if qual is None else bytes(qual)
    assert len(q) == len(seq)
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm), 0, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", c) for c in cigar) + pack_seq(seq) + q + tags
    return struct.pack("<i", len(body)) + body


def header(header_text=b"@HD\tVN:1.5\tSO:unknown\n", refs=()):
    out = b"BAM\1" + struct.pack("<i", len(header_text)) + header_text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def bgzf_block(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    size = 18 + len(body) + 8
    assert size <= 65536 and len(data) <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + body
            + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def bgzf(stream, block_payload=65280, level=6, eof=True, empty_block_every=0):
    """the stream cut into blocks of block_payload inflated bytes wherever they fall; level 0: stored blocks"""
    out = []
    for k, i in enumerate(range(0, len(stream), block_payload)):
        if empty_block_every and k % empty_block_every == empty_block_every - 1:
            out.append(bgzf_block(b"", level))
        out.append(bgzf_block(stream[i:i + block_payload], level))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def bam_stream(reads, quals=None, header_text=b"@HD\tVN:1.5\tSO:unknown\n", refs=(), cigars=None, tags=None, flags=None):
    """the inflated bytes; reads: (name, seq) or [name, seq, ...] of bytes"""
    parts = [header(header_text, refs)]
    for i, r in enumerate(reads):
        parts.append(record(r[0], r[1], quals[i] if quals is not None else None, cigars[i] if cigars is not None else (),
                            tags[i] if tags is not None else b"", flags[i] if flags is not None else 4))
    return b"".join(parts)


def write_bam(path, reads, quals=None, block_payload=65280, level=6, header_text=b"@HD\tVN:1.5\tSO:unknown\n",
              refs=(), cigars=None, tags=None, flags=None, eof=True, empty_block_every=0):
    """-> the inflated bytes of the file written"""
    stream = bam_stream(reads, quals, header_text, refs, cigars, tags, flags)
    with open(path, "wb") as f:
        f.write(bgzf(stream, block_payload, level, eof, empty_block_every))
    return stream
