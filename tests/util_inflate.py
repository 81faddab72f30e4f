"""Helpers of the hostile-stream tests of the device inflater (tests/test_inflate_hostile_host.py on the CPU, tests/test_gpu_read_hostile.py on the
device): a bit writer and stream builder for hand-made zlib streams (RFC 1950 / 1951), the hand-built corpus -- one stream per rule of the decoder,
the smallest that shows it --, the seeded campaign's generators, zlib's verdict on a stream, and the builder of the sanitized CPU program
(tests/c/inflate_hostile_main.cpp).  Nothing here calls the code under test for an expected value: what a stream should do is what zlib does with it."""
import os
import subprocess
import zlib

import numpy as np

from tests import util as U

PLI_IN = 4096                  # the staged input of the shipped kernel (pl_inflate_core.h)
PIECE = 4096                   # what leaves the decoder's window at a time
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---- the bit writer ----

class Bits:
    """a deflate bit stream: fields go in from the lowest bit of a byte on (put), Huffman codes with their first bit first (code)"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        self.v |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        return self

    def code(self, c):
        v, n = c
        return self.put(int(format(v, "0%db" % n)[::-1], 2), n)

    def align(self):
        self.n = (self.n + 7) & ~7
        return self

    def raw(self, data):
        self.align()
        self.v |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)
        return self

    def tobytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canon(lens):
    """code lengths -> {symbol: (code, length)}, the canonical code of RFC 1951 3.2.2"""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    code, nxt = 0, [0] * 17
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


FIXED_L = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)          # (286 and 287 have codes no valid stream uses)
FIXED_D = canon([5] * 32)                                             # (30 and 31 likewise)


def lens_of(assign, n):
    """{symbol: code length} -> the list of n code lengths"""
    out = [0] * n
    for s, l in assign.items():
        out[s] = l
    return out


def head(b, final, btype):
    return b.put(final, 1).put(btype, 2)


def stored(b, data, final=1, length=None, nlen=None):
    length = len(data) if length is None else length
    head(b, final, 0).align().put(length, 16).put(length ^ 0xFFFF if nlen is None else nlen, 16)
    return b.raw(data)


def lits(b, L, data):
    for v in data:
        b.code(L[v])
    return b


def match(b, L, D, length, dist):
    """a length / distance pair in the code sets L and D"""
    i = 28 if length == 258 else max(k for k in range(28) if LBASE[k] <= length)
    b.code(L[257 + i]).put(length - LBASE[i], LEXT[i])
    j = max(k for k in range(30) if DBASE[k] <= dist)
    return b.code(D[j]).put(dist - DBASE[j], DEXT[j])


def dyn_header(b, final, litlens, distlens, cl=None, seq=None, hlit=None, hdist=None, hclen=None):
    """A dynamic block's header.  litlens / distlens: the code lengths; cl: the lengths of the code-length code's 19 symbols (default: 4 bits for
    each of 0..15, no repeat codes); seq: the code-length symbols sent, as (symbol, value of its extra bits) (default: every length by itself);
    hlit / hdist / hclen: the fields' raw values (default: what the lists say)."""
    cl = [4] * 16 + [0, 0, 0] if cl is None else cl
    seq = [(l, 0) for l in list(litlens) + list(distlens)] if seq is None else seq
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl[CLORDER[i]]])
    head(b, final, 2).put(len(litlens) - 257 if hlit is None else hlit, 5).put(len(distlens) - 1 if hdist is None else hdist, 5).put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl[CLORDER[i]], 3)
    C = canon(cl)
    for s, x in seq:
        b.code(C[s]).put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    return b


def zwrap(deflate, expect=None, hdr=b"\x78\x01", tail=b""):
    """header + the deflate bytes + the Adler-32 of what they inflate to (0 where they do not) + tail.  Returns (stream, expect): expect defaults to
    the number of bytes the deflate data holds."""
    deflate = deflate.tobytes() if isinstance(deflate, Bits) else deflate
    try:
        d = zlib.decompressobj(-15)
        data = d.decompress(deflate)
        data = data if d.eof else None
    except zlib.error:
        data = None
    if expect is None:
        assert data is not None, "a stream zlib does not inflate needs its `expect` stated"
        expect = len(data)
    return hdr + deflate + zlib.adler32(data or b"").to_bytes(4, "big") + tail, expect


def zlib_accepts(z, expect):
    """zlib's verdict, as the contract states it: the stream ends (Z_STREAM_END) after exactly `expect` bytes.  Returns the bytes, or None."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(z, expect + 1)
    except zlib.error:
        return None
    if not d.eof and len(out) == expect:           # (an empty final block may still follow the last byte)
        try:
            out += d.decompress(d.unconsumed_tail, 1)
        except zlib.error:
            return None
    return out if d.eof and len(out) == expect else None


# ---- the hand-built corpus ----

# a small complete literal/length set: the literals 0 (an image's first byte: filter type none), a, b, the end code and length code 257 (3 bytes)
_L5 = {0: 2, 97: 2, 98: 2, 256: 3, 257: 3}
# codes of 1 .. 15 bits: literal 0 has 1 bit, 97..107 have 2..12, the end code 13, length code 257 (3 bytes) 14, literal 109 and length code 258 (4 bytes) 15
_LLONG = dict([(0, 1)] + [(97 + i, 2 + i) for i in range(11)] + [(256, 13), (257, 14), (109, 15), (258, 15)])
# distance codes 0..8 of 1..9 bits, 9 and 10 of 10 bits (beyond the 9-bit direct table)
_DLONG = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10]


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _image_bytes(n, seed):
    """n bytes whose first is 0: the scanline of a gray image one row high, filter type none"""
    return b"\x00" + _rand(n - 1, seed) if n else b""


def _plain(nlit, length, dist, prefix=0, bad_dist=None, lit9=False):
    """The start of a fixed-Huffman final block: `nlit` literals and ONE match (both codes in the direct tables); in front of the block `prefix` bytes
    in a stored block.  bad_dist: that distance symbol (30 / 31) in the distance's place.  lit9: the last literal is one of nine bits (the others
    have eight)."""
    b = Bits()
    if prefix:
        stored(b, _image_bytes(prefix, prefix), final=0)
    head(b, 1, 1)
    text = bytearray([98] * nlit)
    if nlit and not prefix:
        text[0] = 0
    if nlit and lit9:
        text[-1] = 200
    lits(b, FIXED_L, bytes(text))
    if bad_dist is None:
        match(b, FIXED_L, FIXED_D, length, dist)
    else:
        i = max(k for k in range(28) if LBASE[k] <= length)
        b.code(FIXED_L[257 + i]).put(length - LBASE[i], LEXT[i]).code(FIXED_D[bad_dist])
    return b


def corpus():
    """The hand-built streams: a list of (name, stream, expect, accept) -- accept is what the case is MEANT to show (the tests check that zlib agrees,
    so that every case is what its name says; the verdict the decoder is held to is zlib's).  One stream per line, the smallest that shows the case."""
    out = []

    def add(name, z, expect, accept):
        out.append((name, bytes(z), expect, accept))

    def addw(name, b, accept, expect=None, **kw):
        z, e = zwrap(b, expect, **kw)
        add(name, z, e, accept)

    def hdr(cmf, flg):
        return bytes([cmf, flg + (31 - ((cmf << 8) + flg) % 31) % 31])

    one, e1 = zwrap(stored(Bits(), b"\x00\x07"))                                                       # 78 01 | 01 02 00 fd ff | 00 07 | Adler-32
    # -- container --
    for k in range(8):
        add("zbytes_%d" % k, one[:k], e1, False)
    add("container_ok", one, e1, True)
    addw("cm_9", stored(Bits(), b"\x00\x07"), False, hdr=hdr(0x79, 0))
    addw("cinfo_8", stored(Bits(), b"\x00\x07"), False, hdr=hdr(0x88, 0))
    addw("fdict", stored(Bits(), b"\x00\x07"), False, hdr=hdr(0x78, 0x20))
    addw("fcheck_off_by_one", stored(Bits(), b"\x00\x07"), False, hdr=b"\x78\x02")
    for k in range(4):
        add("trailer_cut_after_%d" % k, one[:len(one) - 4 + k], e1, False)
    add("garbage_behind_trailer", one + b"\xff", e1, True)
    add("adler_off_by_one_bit", one[:-1] + bytes([one[-1] ^ 1]), e1, False)
    add("adler_off_in_its_first_byte", one[:-4] + bytes([one[-4] ^ 0x80]) + one[-3:], e1, False)
    # -- stored blocks --
    addw("stored_len_nlen_mismatch", stored(Bits(), b"\x00ab", nlen=3 ^ 0xFFFE), False, expect=3)
    addw("stored_len_0_then_data", stored(stored(Bits(), b"", final=0), b"\x00ab"), True)
    addw("stored_len_0_final_behind_data", stored(stored(Bits(), b"\x00ab", final=0), b""), True)
    addw("stored_len_65535", stored(Bits(), _image_bytes(65535, 1)), True)
    addw("stored_len_one_more_than_expect_leaves", stored(stored(Bits(), b"\x00ab", final=0), b"cde"), False, expect=5)
    addw("stored_len_exactly_what_expect_leaves", stored(stored(Bits(), b"\x00ab", final=0), b"cde"), True, expect=6)
    st, _ = zwrap(stored(Bits(), b"\x00abcdefg"))
    add("stored_cut_inside_len", st[:4], 8, False)
    add("stored_cut_inside_nlen", st[:6], 8, False)
    add("stored_cut_inside_payload", st[:11], 8, False)
    for turn in (1, 3):
        for inside in (4, 3, 2, 1, 0):
            n = PLI_IN * turn + (4 - inside) - 11                                                   # a stored stream of n bytes is n + 11 long
            addw("stored_final_trailer_%d_inside_stage_%d" % (inside, turn), stored(Bits(), _image_bytes(n, n)), True)
    addw("stored_behind_huffman_block_ending_mid_byte", stored(lits(head(Bits(), 0, 1), FIXED_L, b"\x00ab").code(FIXED_L[256]), b"cde"), True)
    # -- dynamic headers --
    L5, D2 = lens_of(_L5, 258), [1, 1]
    CD2 = canon(D2)
    C5 = canon(L5)

    def body5(b, D=CD2):                                                                           # 0 a b, a match of three at distance 2, the end code
        return match(lits(b, C5, b"\x00ab"), C5, D, 3, 2).code(C5[256])

    dyn_ok = body5(dyn_header(Bits(), 1, L5, D2))
    addw("dynamic_ok", dyn_ok, True)
    for n in (287, 288):
        addw("hlit_%d" % n, body5(dyn_header(Bits(), 1, L5 + [0] * (n - 258), D2)), False, expect=6)
    for n in (31, 32):
        addw("hdist_%d" % n, body5(dyn_header(Bits(), 1, L5, D2 + [0] * (n - 2))), False, expect=6)
    addw("hlit_286_hdist_30", body5(dyn_header(Bits(), 1, L5 + [0] * 28, D2 + [0] * 28)), True)
    addw("hclen_4_all_zero", dyn_header(Bits(), 1, L5, D2, cl=[0] * 19, seq=[]).put(0, 64), False, expect=6)
    addw("code_length_code_over_subscribed", dyn_header(Bits(), 1, L5, D2, cl=[1, 1, 1] + [0] * 16, seq=[]).put(0, 64), False, expect=6)
    addw("code_length_code_over_subscribed_late", dyn_header(Bits(), 1, L5, D2, cl=[1, 2, 3, 4, 5, 6, 7, 7, 7] + [0] * 10, seq=[]).put(0, 64), False, expect=6)
    addw("code_length_code_incomplete", dyn_header(Bits(), 1, L5, D2, cl=[1, 2] + [0] * 17, seq=[]).put(0, 64), False, expect=6)
    for s in (0, 2, 8, 17, 18):
        addw("code_length_code_single_code_%d" % s, dyn_header(Bits(), 1, L5, D2, cl=[1 if k == s else 0 for k in range(19)], seq=[(s, 0)] * 260).put(0, 64), False, expect=6)
    clr = [5] * 16 + [2, 3, 3]                                                                     # a code-length code with the three repeat codes
    addw("repeat_16_first", body5(dyn_header(Bits(), 1, L5, D2, cl=clr, seq=[(16, 0)] + [(l, 0) for l in L5[3:] + D2])), False, expect=6)
    plain = [(l, 0) for l in L5 + D2]
    addw("repeat_16_of_a_zero_length", body5(dyn_header(Bits(), 1, L5, D2, cl=clr, seq=plain[:2] + [(16, 0)] + plain[5:])), True)
    L7 = lens_of({0: 2, 97: 3, 98: 3, 99: 3, 100: 3, 256: 3, 257: 3}, 258)
    b = dyn_header(Bits(), 1, L7, D2, cl=clr, seq=[(l, 0) for l in L7[:98]] + [(16, 0)] + [(l, 0) for l in L7[101:] + D2])
    addw("repeat_16_of_a_code_length", match(lits(b, canon(L7), b"\x00abcd"), canon(L7), CD2, 3, 2).code(canon(L7)[256]), True)
    L5z = lens_of(_L5, 262)
    # 258 + 4 lengths, the last three a repeat of zero that starts at the last but one: one too many; with a fifth distance length it ends where the lengths do
    addw("repeat_runs_past_the_end_by_one", body5(dyn_header(Bits(), 1, L5, [1, 1, 0, 0], cl=clr, seq=plain + [(17, 0)])), False, expect=6)
    addw("repeat_ends_where_the_lengths_end", body5(dyn_header(Bits(), 1, L5, [1, 1, 0, 0, 0], cl=clr, seq=plain + [(17, 0)])), True)
    CD_23 = canon([0, 0, 1, 1])
    b = dyn_header(Bits(), 1, L5z[:260], [0, 0, 1, 1], cl=clr, seq=[(l, 0) for l in L5z[:258]] + [(17, 1)] + [(1, 0), (1, 0)])
    addw("repeat_crosses_from_literal_into_distance_lengths", match(lits(b, C5, b"\x00ab"), C5, CD_23, 3, 3).code(C5[256]), True)
    b = dyn_header(Bits(), 1, L5z[:260], [0, 0, 1, 1], cl=clr, seq=[(l, 0) for l in L5z[:257]] + [(3, 0), (18, 127)])
    addw("repeat_18_runs_past_the_end", b.put(0, 64), False, expect=6)
    addw("no_end_of_block_code", lits(dyn_header(Bits(), 1, lens_of({0: 1, 97: 1}, 258), D2), canon(lens_of({0: 1, 97: 1}, 258)), b"\x00a").put(0, 64), False, expect=2)
    addw("literal_set_over_subscribed", dyn_header(Bits(), 1, lens_of({0: 1, 97: 1, 256: 1}, 258), D2).put(0, 64), False, expect=2)
    addw("literal_set_incomplete", dyn_header(Bits(), 1, lens_of({0: 2, 97: 2, 256: 2}, 258), D2).put(0, 64), False, expect=2)
    L3 = lens_of({0: 1, 97: 2, 256: 2}, 257)
    addw("distance_set_of_no_code", lits(dyn_header(Bits(), 1, L3, [0]), canon(L3), b"\x00aa").code(canon(L3)[256]), True)
    addw("distance_set_of_one_1_bit_code", body5(dyn_header(Bits(), 1, L5, [0, 1]), canon([0, 1])), True)
    addw("distance_set_of_one_1_bit_code_the_other_code_used", lits(dyn_header(Bits(), 1, L5, [0, 1]), C5, b"\x00ab").code(C5[257]).put(1, 1).code(C5[256]), False, expect=6)
    addw("distance_set_of_one_2_bit_code", body5(dyn_header(Bits(), 1, L5, [0, 2]), canon([0, 2])), False, expect=6)
    addw("distance_set_of_two_1_bit_codes", body5(dyn_header(Bits(), 1, L5, [0, 1, 1]), canon([0, 1, 1])), True)
    z, e = zwrap(dyn_ok)
    hb = (dyn_header(Bits(), 1, L5, D2).n + 7) // 8
    for k in range(2, 2 + hb + 1):
        add("dynamic_header_cut_at_byte_%d" % k, z[:k], e, False)
    add("dynamic_block_cut_before_trailer", z[:-4], e, False)
    # -- symbols --
    for s in (286, 287):
        addw("fixed_length_code_%d" % s, lits(head(Bits(), 1, 1), FIXED_L, b"\x00ab").code(FIXED_L[s]).put(0, 64), False, expect=6)
    for s in (30, 31):
        addw("fixed_distance_code_%d" % s, _plain(3, 3, 1, bad_dist=s).put(0, 64), False, expect=6)
    LL, DL = lens_of(_LLONG, 259), _DLONG
    CL, CDL = canon(LL), canon(DL)
    far = b"\x00" + bytes([97 + (i * 7) % 11 for i in range(39)])
    b = lits(dyn_header(Bits(), 1, LL, DL), CL, far + b"m")                                        # m = 109: a literal of 15 bits
    match(b, CL, CDL, 3, 40)                                                                       # length code of 14 bits, distance code 10 (33..48) of 10 bits
    match(b, CL, CDL, 4, 25)                                                                       # length code of 15 bits, distance code 9 (25..32) of 10 bits
    match(b, CL, CDL, 3, 1)                                                                        # length code of 14 bits, distance code of 1 bit
    addw("long_codes_literal_length_distance", b.code(CL[256]), True)
    b = lits(dyn_header(Bits(), 1, LL, DL), CL, far)
    addw("long_length_code_long_distance_beyond_the_bytes_produced", match(b, CL, CDL, 4, 41).code(CL[256]), False, expect=44)
    addw("long_length_code_match_end_beyond_expect", match(lits(dyn_header(Bits(), 1, LL, DL), CL, far), CL, CDL, 4, 40).code(CL[256]), False, expect=43)
    LU = lens_of(dict([(0, 1)] + [(97 + i, 2 + i) for i in range(11)] + [(256, 13), (257, 13)]), 258)         # (complete: 1/2 + ... + 2^-12 + 2 * 2^-13)
    b = lits(dyn_header(Bits(), 1, LU, [0, 1]), canon(LU), b"\x00ab").code(canon(LU)[257]).put(1, 1)
    addw("unassigned_distance_code_behind_a_long_length_code", b.put(0, 64), False, expect=6)
    addw("no_end_code_before_the_input_ends", lits(head(Bits(), 1, 1), FIXED_L, b"\x00abcdefgh"), False, expect=9)
    add("no_end_code_and_no_trailer", b"\x78\x01" + lits(head(Bits(), 1, 1), FIXED_L, b"\x00abcdefgh").tobytes(), 9, False)
    # -- the plain-match path: one rule broken at a time, by the smallest amount, with 0..38 literals in front of the match in the same block, and with the match
    #    crossing a 4096-byte piece boundary --
    for nlit in range(0, 39):
        tag = "_behind_%d_literals" % nlit
        addw("distance_is_bytes_produced_plus_1" + tag, _plain(nlit, 3, nlit + 1).code(FIXED_L[256]), False, expect=nlit + 3)
        addw("distance_kind_bad_behind_a_good_length" + tag, _plain(nlit, 3, 1, bad_dist=30).put(0, 64), False, expect=nlit + 3)
        if not nlit:
            continue
        # the match's last bit is the stream's last bit (no end code, no trailer: the stream ends there), and lies one bit past it.  Behind 5 literals and more a match
        # of 3 at distance 5: 3 + 8 nlit + 7 + 5 + 1 bits, the last one the distance's extra bit; in front of that a match of 11 at distance 1: 3 + 8 nlit + 7 + 1 + 5.
        # With one literal of nine bits the match ends one bit into a further byte, and that byte is cut
        for lit9 in (False, True):
            b = _plain(nlit, 3, 5, lit9=lit9) if nlit >= 5 else _plain(nlit, 11, 1, lit9=lit9)
            assert b.n % 8 == (1 if lit9 else 0)
            z = b"\x78\x01" + b.tobytes()
            add(("match_ends_one_bit_past_the_streams_last" if lit9 else "match_ends_with_the_streams_last_bit") + tag, z[:-1] if lit9 else z, nlit + (3 if nlit >= 5 else 11), False)
        addw("distance_is_bytes_produced" + tag, _plain(nlit, 3, nlit).code(FIXED_L[256]), True)
        addw("match_end_is_expect" + tag, _plain(nlit, 9, 1).code(FIXED_L[256]), True)
        addw("match_end_is_expect_plus_1" + tag, _plain(nlit, 9, 1).code(FIXED_L[256]), False, expect=nlit + 8)
        addw("length_64" + tag, _plain(nlit, 64, 1).code(FIXED_L[256]), True)
        addw("length_65" + tag, _plain(nlit, 65, 1).code(FIXED_L[256]), True)
        pre = PIECE - nlit - 2                                                                     # the match starts two bytes in front of the boundary
        addw("match_crosses_piece" + tag, _plain(nlit, 64, 7, prefix=pre).code(FIXED_L[256]), True)
        addw("match_crosses_piece_distance_is_bytes_produced" + tag, _plain(nlit, 5, pre + nlit, prefix=pre).code(FIXED_L[256]), True)
        addw("match_crosses_piece_distance_is_bytes_produced_plus_1" + tag, _plain(nlit, 5, pre + nlit + 1, prefix=pre).code(FIXED_L[256]), False, expect=pre + nlit + 5)
        addw("match_crosses_piece_end_is_expect_plus_1" + tag, _plain(nlit, 5, 3, prefix=pre).code(FIXED_L[256]), False, expect=pre + nlit + 4)
        addw("match_crosses_piece_length_65" + tag, _plain(nlit, 65, 9, prefix=pre).code(FIXED_L[256]), True)
    for nlit in (0, 1, 2, 17, 37, 38):
        tag = "_behind_%d_literals" % nlit
        for length in (3, 64):
            addw("distance_plus_length_32768_length_%d" % length + tag, _plain(nlit, length, 32768 - length, prefix=32768).code(FIXED_L[256]), True)
            addw("distance_plus_length_32769_length_%d" % length + tag, _plain(nlit, length, 32769 - length, prefix=32768).code(FIXED_L[256]), True)
    # -- runs of literals --
    run = b"\x00" + bytes(range(1, 60))
    addw("literal_run_ends_at_expect", lits(head(Bits(), 1, 1), FIXED_L, run).code(FIXED_L[256]), True)
    addw("literal_run_ends_one_past_expect", lits(head(Bits(), 1, 1), FIXED_L, run).code(FIXED_L[256]), False, expect=len(run) - 1)
    for pre in (PIECE - 1, PIECE - 20, PIECE - 59):
        addw("literal_run_crosses_piece_from_%d" % pre, lits(head(stored(Bits(), _image_bytes(pre, pre), final=0), 1, 1), FIXED_L, run[1:]).code(FIXED_L[256]), True)
    La = lens_of({0: 1, 97: 2, 256: 2}, 257)                                                       # (the code of all zero bits is a literal: what the zero padding decodes to)
    add("literal_run_from_the_padding_behind_the_streams_last_byte", b"\x78\x01" + lits(dyn_header(Bits(), 1, La, [0]), canon(La), b"\x00aa\x00").tobytes(), 64, False)
    # -- nothing at all --
    addw("expect_0_empty_fixed_block", head(Bits(), 1, 1).code(FIXED_L[256]), True)
    addw("expect_0_empty_stored_block", stored(Bits(), b""), True)
    addw("expect_0_but_one_byte", stored(Bits(), b"\x00\x07"), False, expect=0)
    assert len({c[0] for c in out}) == len(out)
    return out


# ---- the seeded campaign ----

def _payload(rng, n):
    kind = int(rng.integers(0, 4))
    if kind == 0:                                            # noise
        a = rng.integers(0, 256, n, dtype=np.uint8)
    elif kind == 1:                                          # a smooth walk
        a = (np.cumsum(rng.integers(-2, 3, n)) % 256).astype(np.uint8)
    elif kind == 2:                                          # mostly constant
        a = np.full(n, int(rng.integers(0, 256)), np.uint8)
        k = max(1, n // 50)
        a[rng.integers(0, n, k)] = rng.integers(0, 256, k, dtype=np.uint8)
    else:                                                    # a skewed alphabet (codes of 2 to 15 bits) with short copies
        a = np.minimum(255, rng.geometric(0.06, n)).astype(np.uint8)
        for _ in range(n // 200):
            s, d, l = (int(v) for v in (rng.integers(0, n), rng.integers(0, n), rng.integers(3, 70)))
            l = min(l, n - s, n - d)
            a[d:d + l] = a[s:s + l].copy()
    return a.tobytes()


MUTATIONS = ("none", "one bit", "three bits", "one byte", "a bit in the first 40 bytes", "truncation", "a byte appended", "expect off")


def _flip(z, rng, lo, hi):
    z = bytearray(z)
    if z:
        i = int(rng.integers(lo, max(lo + 1, min(hi, len(z)))))
        if i < len(z):
            z[i] ^= 1 << int(rng.integers(0, 8))
    return bytes(z)


def campaign_compressed(seed, count):
    """The first generator: payloads of four kinds of 1..3000 bytes (one in four up to 70 000), zlib at levels 0 / 1 / 6 / 9, its five strategies, window
    bits 9..15, then one of the eight mutations.  Returns [(stream, expect, mutation index)].  Deterministic."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(1, 70001)) if int(rng.integers(0, 4)) == 0 else int(rng.integers(1, 3001))
        data = _payload(rng, n)
        co = zlib.compressobj(int(rng.choice([0, 1, 6, 9])), zlib.DEFLATED, int(rng.integers(9, 16)), 8,
                              int(rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])))
        z = co.compress(data) + co.flush()
        expect, m = n, int(rng.integers(0, 8))
        if m == 1:
            z = _flip(z, rng, 0, len(z))
        elif m == 2:
            for _ in range(3):
                z = _flip(z, rng, 0, len(z))
        elif m == 3:
            b = bytearray(z)
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            z = bytes(b)
        elif m == 4:
            z = _flip(z, rng, 0, 40)
        elif m == 5:
            z = z[:int(rng.integers(0, len(z)))]
        elif m == 6:
            z = z + bytes([int(rng.integers(0, 256))])
        elif m == 7:
            expect = max(0, n + int(rng.choice([-2, -1, 1, 2])))
        out.append((z, expect, m))
    return out


def campaign_random_blocks(seed, count):
    """The second generator: 78 9c, then random bytes whose first three bits are forced to a final fixed or dynamic block.  Where the deflate data is
    sound (zlib's only complaint would be the data check) the stream is cut behind it and given its Adler-32, so that accepted dynamic blocks occur.
    Returns [(stream, expect, 8)].  Deterministic."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        body = bytearray(rng.integers(0, 256, int(rng.integers(4, 400)), dtype=np.uint8).tobytes())
        body[0] = (body[0] & 0xF8) | 1 | (int(rng.integers(1, 3)) << 1)
        body = bytes(body)
        z, expect = b"\x78\x9c" + body, int(rng.integers(0, 300))
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(body, 1 << 20)
            if d.eof:
                z = b"\x78\x9c" + body[:len(body) - len(d.unused_data)] + zlib.adler32(data).to_bytes(4, "big")
                expect = len(data) if int(rng.integers(0, 8)) else max(0, len(data) + int(rng.choice([-1, 1])))
        except zlib.error:
            pass
        out.append((z, expect, 8))
    return out


# ---- tests/c/inflate_hostile_main.cpp: the core on the CPU, under the sanitizers ----

SANITIZE = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build_hostile(tmp_path, name, defs=()):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17"] + SANITIZE + list(defs) + ["-o", exe, os.path.join(U.ROOT, "tests", "c", "inflate_hostile_main.cpp"), "-lz"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_sanitized(cmd, timeout=300):
    """Runs a sanitized program: fails on a non-zero exit and on any sanitizer report.  Returns its standard output."""
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def run_hostile(exe, tmp_path, cases, tag="cases"):
    """cases: (stream, expect).  Returns per case (core status, zlib accepts, verdict) as tests/c/inflate_hostile_main.cpp words them."""
    path, res = str(tmp_path / (tag + ".bin")), str(tmp_path / (tag + ".txt"))
    with open(path, "wb") as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for z, expect in cases:
            fh.write(np.array([len(z), expect], np.uint32).tobytes())
            fh.write(z)
    run_sanitized([exe, path, res])
    with open(res) as fh:
        rows = [ln.split() for ln in fh]
    assert len(rows) == len(cases)
    return [(int(a), int(b), c) for a, b, c in rows]
