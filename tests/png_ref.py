"""A numpy model of the project's PNG encoder (include/gftorf_png.h, csrc/k_png.hip, csrc/gft_png_coder.h).

It restates the header's rules one by one -- the filter choice per scanline, the cut into segments, the five candidate
distances and the hash candidate, the greedy parse, deflate's fixed Huffman codes from the tables of RFC 1951, the stored fallback, one IDAT chunk
per segment, the closing chunk with the Adler-32 -- in plain numpy and Python, with zlib's crc32 and adler32 for the check
sums.  It needs no device.  The reference project has no encoder (it calls imageio); this is the specification the kernels
are held to, byte for byte (tests/test_png.py), and the file it writes is checked on its own against Pillow and zlib
(tests/test_png_ref.py).
"""
import functools
import struct
import zlib

import numpy as np

SEGMENT = 32768
MAX_MATCH, MIN_MATCH = 258, 3
HASH_BITS, HASH_MIN, HASH_MAX = 12, 4, 7          # the sixth candidate: buckets, least and greatest length
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}

# RFC 1951, 3.2.5
LENGTH_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LENGTH_EXTRA = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
DIST_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                      8193, 12289, 16385, 24577])
DIST_EXTRA = np.array([0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13])


def as_image(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.uint8 and a.ndim in (2, 3), (a.dtype, a.shape)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.shape[2] in COLOUR_TYPE and a.shape[0] >= 1 and a.shape[1] >= 1, a.shape
    return a


def segments_of(total):
    return (total + SEGMENT - 1) // SEGMENT


def bound(H, W, C):
    """gft_png_bound: the size of a level-0 file and the upper bound of a level-1 file"""
    total = H * (1 + W * C)
    return 8 + 25 + 2 + segments_of(total) * (12 + 5) + total + 21 + 12


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def filter_rows(a):
    """the rows filtered with types 0, 1 and 2: uint8 [3, H, W * C]"""
    H, W, C = a.shape
    raw = a.reshape(H, W * C)
    left = np.zeros_like(raw)
    left[:, C:] = raw[:, :-C]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    return np.stack([raw, raw - left, raw - up])            # uint8 arithmetic wraps


def filter_types(a, level):
    """per scanline 0, 1 or 2: the least sum of the filtered bytes read as signed magnitudes, ties to the lowest type"""
    a = as_image(a)
    if level == 0:
        return np.zeros(a.shape[0], np.uint8)
    f = filter_rows(a).astype(np.int64)
    cost = np.where(f < 128, f, 256 - f).sum(axis=2)        # [3, H]
    return np.argmin(cost, axis=0).astype(np.uint8)         # argmin takes the first of equals


def filtered_stream(a, types):
    a = as_image(a)
    f = filter_rows(a)
    H = a.shape[0]
    rows = f[types.astype(np.int64), np.arange(H)]          # [H, W * C]
    return np.concatenate([types.reshape(H, 1), rows], axis=1).reshape(-1)


def hash_candidate(seg):
    """(length, distance) of the sixth candidate for every byte: the least position whose four bytes fall into the same bucket,
    where that lies in front of j; the length cut at HASH_MAX and at the segment's end; (0, 0) where there is none"""
    n = len(seg)
    length, dist = np.zeros(n, np.int64), np.zeros(n, np.int64)
    m = n - HASH_MIN + 1
    if m <= 0:
        return length, dist
    s = seg.astype(np.uint32)
    g = s[0:m] | (s[1:m + 1] << np.uint32(8)) | (s[2:m + 2] << np.uint32(16)) | (s[3:m + 3] << np.uint32(24))
    bucket = ((g * np.uint32(2654435761)) >> np.uint32(32 - HASH_BITS)).astype(np.int64)       # uint32 arithmetic wraps
    first = np.full(1 << HASH_BITS, n, np.int64)
    np.minimum.at(first, bucket, np.arange(m))
    j = np.arange(m)
    p = first[bucket]
    alive = p < j
    for k in range(HASH_MAX):
        alive = alive & (j + k < n)
        alive[alive] = seg[j[alive] + k] == seg[p[alive] + k]
        length[:m] += alive
    dist[:m] = np.where(p < j, j - p, 0)
    return length, dist


def best_matches(seg, L):
    """(length, candidate, distance) for every byte of a segment: candidates 1, 2, 3, 4, L in this order, the longest wins, ties
    to the earlier; length 0 where j < d, runs cut at 258 and at the segment's end; candidate 5 is the hash candidate, which
    wins only with a length of HASH_MIN or more that is greater than the others'"""
    n = len(seg)
    runs = np.zeros((5, n), np.int64)
    j = np.arange(n)
    for q, d in enumerate((1, 2, 3, 4, L)):
        if d >= n:
            continue
        eq = np.zeros(n, bool)
        eq[d:] = seg[d:] == seg[:-d]
        stop = np.where(~eq, j, n)                          # the next j' >= j with eq false
        stop = np.minimum.accumulate(stop[::-1])[::-1]
        runs[q] = np.minimum(stop - j, MAX_MATCH)
    length, cand = runs.max(axis=0), runs.argmax(axis=0)
    dist = np.array([1, 2, 3, 4, L], np.int64)[cand]
    hlen, hdist = hash_candidate(seg)
    use = (hlen >= HASH_MIN) & (hlen > length)
    return np.where(use, hlen, length), np.where(use, 5, cand), np.where(use, hdist, dist)


def parse(seg, L):
    """the greedy parse: arrays (position, length or 0 for a literal, candidate, distance) of the tokens"""
    length, cand, dist = best_matches(seg, L)
    n = len(seg)
    step = np.where(length >= MIN_MATCH, length, 1)
    nxt = (np.arange(n) + step).tolist()
    at, j = [], 0
    while j < n:
        at.append(j)
        j = nxt[j]
    assert j == n
    at = np.array(at, np.int64)
    ln = np.where(length[at] >= MIN_MATCH, length[at], 0)
    return at, ln, cand[at], dist[at]


def reverse_bits(v, n):
    out = np.zeros_like(v)
    for k in range(int(np.max(n, initial=0))):
        out |= np.where(k < n, ((v >> k) & 1) << np.maximum(n - 1 - k, 0), 0)
    return out


def litlen_code(sym):
    """fixed Huffman code of literal/length symbols, RFC 1951 3.2.6: (code, bits)"""
    code = np.select([sym < 144, sym < 256, sym < 280], [0x30 + sym, 0x190 + sym - 144, sym - 256], 0xc0 + sym - 280)
    bits = np.select([sym < 144, sym < 256, sym < 280], [8, 9, 7], 8)
    return code, bits


def token_bits(seg, at, ln, dist):
    """per token the bits as they enter the stream from bit 0 up (uint64) and their count: Huffman codes most significant bit
    first, extra bits least significant first"""
    lit = ln == 0
    lidx = np.searchsorted(LENGTH_BASE, np.where(lit, 3, ln), side="right") - 1
    sym = np.where(lit, seg[at].astype(np.int64), 257 + lidx)
    code, nb = litlen_code(sym)
    val = reverse_bits(code, nb).astype(np.uint64)
    count = nb.copy()
    lext = np.where(lit, 0, LENGTH_EXTRA[lidx])
    val |= (np.where(lit, 0, ln - LENGTH_BASE[lidx]).astype(np.uint64) << count.astype(np.uint64))
    count += lext
    didx = np.searchsorted(DIST_BASE, np.where(lit, 1, dist), side="right") - 1
    dcode = reverse_bits(didx, np.full_like(didx, 5)).astype(np.uint64)
    val |= np.where(lit, 0, dcode << count.astype(np.uint64)).astype(np.uint64)
    count += np.where(lit, 0, 5)
    dext = np.where(lit, 0, dist - DIST_BASE[didx]).astype(np.uint64)
    val |= np.where(lit, 0, dext << count.astype(np.uint64)).astype(np.uint64)
    count += np.where(lit, 0, DIST_EXTRA[didx])
    return val, count


def pack_bits(val, count, lead_bits, lead_count):
    """the byte string of `lead_bits` followed by the tokens' bits, padded with zero bits to a byte boundary"""
    val = np.concatenate([np.array([lead_bits], np.uint64), val])
    count = np.concatenate([np.array([lead_count], np.int64), count])
    start = np.concatenate([[0], np.cumsum(count)])
    tok = np.repeat(np.arange(len(val)), count)
    bitno = (np.arange(start[-1]) - start[tok]).astype(np.uint64)
    bits = ((val[tok] >> bitno) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes()


def stored_form(seg):
    n = len(seg)
    return b"\x00" + struct.pack("<HH", n & 0xffff, ~n & 0xffff) + seg.tobytes()


def fixed_form(seg, L):
    """a non-final fixed-Huffman block, its end-of-block code, an empty non-final stored block; and the token count"""
    at, ln, cand, dist = parse(seg, L)
    val, count = token_bits(seg, at, ln, dist)
    total = 3 + int(count.sum()) + 7 + 3
    nbytes = (total + 7) // 8 + 4
    if nbytes > 5 + len(seg):
        return None, nbytes, len(at)                        # not taken: no need to pack it
    body = pack_bits(val, count, 2, 3)                      # BFINAL 0, BTYPE 01; then the tokens
    body = body + b"\x00" * ((total + 7) // 8 - len(body))  # the end-of-block code and the stored header are zero bits
    return body + b"\x00\x00\xff\xff", nbytes, len(at)


def encode_parts(a, level=1):
    """{"file", "types", "stream", "chunks": the segment chunks' whole bytes, "forms": "fixed" / "stored" per segment}"""
    assert level in (0, 1)
    a = as_image(a)
    H, W, C = a.shape
    L = 1 + W * C
    types = filter_types(a, level)
    stream = filtered_stream(a, types)
    chunks, forms = [], []
    for s in range(segments_of(len(stream))):
        seg = stream[s * SEGMENT:(s + 1) * SEGMENT]
        data, form = stored_form(seg), "stored"
        if level >= 1:
            fixed, nbytes, _ = fixed_form(seg, L)
            if fixed is not None:
                assert len(fixed) == nbytes <= len(data)
                data, form = fixed, "fixed"
        chunks.append(chunk(b"IDAT", (b"\x78\x01" if s == 0 else b"") + data))
        forms.append(form)
    closing = chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xffffffff))
    ihdr = chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[C], 0, 0, 0))
    file = SIGNATURE + ihdr + b"".join(chunks) + closing + chunk(b"IEND", b"")
    return {"file": file, "types": types, "stream": stream, "chunks": chunks, "forms": forms}


def encode(a, level=1):
    return encode_parts(a, level)["file"]


# ---- reading a file back without a PNG library -----------------------------------------------------------------------------

def walk_chunks(data):
    """[(kind, data)] of a file; asserts the signature, every length and every CRC"""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(body) == n, (kind, n)
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xffffffff, kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[0][0] == b"IHDR" and out[-1] == (b"IEND", b"")
    return out


def decode(data):
    """the image of a file of this encoder's kind (8 bit, colour type 0 / 2 / 6, filters 0..2), with zlib and numpy alone"""
    chunks = walk_chunks(data)
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    C = {v: k for k, v in COLOUR_TYPE.items()}[colour]
    assert all(k == b"IDAT" for k, _ in chunks[1:-1])
    stream = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks[1:-1])), np.uint8)
    assert len(stream) == H * (1 + W * C)
    rows = stream.reshape(H, 1 + W * C)
    out = np.zeros((H, W * C), np.uint8)
    for y in range(H):
        t, f = int(rows[y, 0]), rows[y, 1:]
        if t == 0:
            out[y] = f
        elif t == 1:
            out[y] = np.cumsum(f.reshape(W, C).astype(np.int64), axis=0).reshape(-1) & 255
        elif t == 2:
            out[y] = f + (out[y - 1] if y else 0)
        else:
            raise AssertionError("filter type %d" % t)
    return out.reshape(H, W, C) if C > 1 else out.reshape(H, W)


# ---- the shapes and contents both test files use ----------------------------------------------------------------------------

SHAPES = [(1, 1, 1), (1, 1, 3), (1, 1, 4), (3, 5, 3), (7, 333, 1), (32, 1023, 1), (33, 1023, 1), (16, 4112, 3), (2, 8200, 4),
          (240, 320, 1), (240, 320, 3), (240, 320, 4)]
CONTENTS = ["zeros", "ones", "ramp", "noise", "half", "period3", "period4", "grain"]


def content(name, shape, seed=0):
    H, W, C = shape
    n = H * W * C
    rng = np.random.default_rng(seed + 1000 * H + 10 * W + C)
    if name == "zeros":
        a = np.zeros(n, np.uint8)
    elif name == "ones":
        a = np.full(n, 255, np.uint8)
    elif name == "ramp":
        a = ((np.arange(W)[None, :, None] + 2 * np.arange(H)[:, None, None] + 7 * np.arange(C)[None, None, :]) & 255).astype(np.uint8)
    elif name == "noise":
        a = rng.integers(0, 256, n, dtype=np.uint8)
    elif name == "half":
        a = np.full((H, W * C), 77, np.uint8)
        a[:(H + 1) // 2] = rng.integers(0, 256, ((H + 1) // 2, W * C), dtype=np.uint8)
    elif name == "grain":                                   # few values at random: repeats at any distance, the hash candidate's
        a = rng.integers(0, 3, n, dtype=np.uint8) * 7
    elif name == "period3":
        a = np.array([5, 200, 91], np.uint8)[np.arange(n) % 3]
    elif name == "period4":
        a = np.array([1, 2, 3, 250], np.uint8)[np.arange(n) % 4]
    else:
        raise KeyError(name)
    a = np.ascontiguousarray(a.reshape(H, W, C))
    return a[:, :, 0] if C == 1 else a


@functools.lru_cache(maxsize=None)
def case(name, shape, level):
    """(image, the model's parts) of a test case, computed once per process; treat both as read-only"""
    a = content(name, shape)
    a.setflags(write=False)
    return a, encode_parts(a, level)
