"""Directed lzip members, written bit by bit with tests/lzma_directed.py's range encoder and LZMA symbol encoder (its Lzma2
chunker writes the parse; the chunk's header is taken off, and the End Of Stream marker is one more match, of distance 2^32),
each named for what it reaches in lzip_member.h, xz_stream.h's lzma_run<true> and lzip_walk.h.  A file is the directed member
-- `@CO` lines, skipped with the header -- and, behind it, a member with the SAM header and the records.  The refused ones
break one rule each in an otherwise good file.  Test infrastructure only."""
import struct

from tests import lzma_directed as D
from tests import sam_lzip as Z
from tests.lzma_directed import SHORTREP, lit, match

MARKER = match(1 << 32, 2)


def stream(ops, dict_size=1 << 16, marker=MARKER):
    """(the LZMA stream of the parse `ops` with the marker behind it, the text): one chunk of D.Lzma2 without its 6-byte header."""
    z = D.Lzma2(dict_size, valid=False)
    z.lzma(list(ops) + ([marker] if marker else []), 0xe0, (3, 0, 2))
    text = bytes(z.text[:len(z.text) - marker[2]]) if marker else bytes(z.text)   # (the marker "copies" its length: not text)
    return z.chunks[0][6:], text


def member_of(ops, dict_size=1 << 16, ds=None, marker=MARKER, stated=None):
    """(a member of the parse, its text); stated: the text the trailer speaks of when not the parse's."""
    data, text = stream(ops, dict_size, marker)
    ds = Z.ds_byte_of(dict_size) if ds is None else ds
    return Z.wrap(data, text if stated is None else stated, ds), text


# ---- a legal header inside a member's payload
def _literal(state, byte):
    """One plain literal (state 0, lc 3) through the range encoder; state: (rc, literal probabilities, is_match probabilities, text)."""
    rc0, lits, is_match, t = state
    rc = D._Rc()
    rc.low, rc.range, rc.cache, rc.pending, rc.out = rc0.low, rc0.range, rc0.cache, rc0.pending, bytearray(rc0.out)
    lits, is_match = list(lits), list(is_match)
    rc.bit(is_match, len(t) & 3, 0)
    base, sym = 0x300 * ((t[-1] if t else 0) >> 5), 1
    for k in range(7, -1, -1):
        b = (byte >> k) & 1
        rc.bit(lits, base + sym, b)
        sym = (sym << 1) | b
    return rc, lits, is_match, t + bytes([byte])


def _reach(state):
    """The first and the last output the encoder can still end in."""
    out = []
    for top in (0, 1):
        rc0 = state[0]
        rc = D._Rc()
        rc.low, rc.range, rc.cache, rc.pending, rc.out = rc0.low + top * (rc0.range - 1), rc0.range, rc0.cache, rc0.pending, bytearray(rc0.out)
        out.append(rc.finish())
    return out


def planted_literals(prefix: bytes, target: bytes):
    """(the prefix, with fillers; the literals; the stream offset): behind the literals `prefix`, literals whose range-coded bytes are `target`.  Probabilities
    near 1024 code a literal's bits at about a bit each -- raw, as good as --, so a literal pins about a byte of the output: a
    depth-first search over literal values keeps those whose reachable outputs still hold the target."""
    state = (D._Rc(), [1024] * (0x300 << 3), [1024] * 192, b"")
    for byte in prefix:
        state = _literal(state, byte)
    # (a literal starts with the is_match bit: the prefix must be long enough to have made a literal all but certain there,
    # or the target falls to the matches' share of the range at some depth)
    # the output so far is settled up to where the two ends part; the byte there can still take the values in between, and
    # behind such a value every byte is free: the whole output is to start with `want`
    while True:
        a, b = _reach(state)
        c = next(k for k in range(len(a)) if a[k] != b[k])
        if b[c] - a[c] >= 2:
            break
        state = _literal(state, ord("."))   # (the two ends part by one: nothing in between; a filler moves them)
        prefix += b"."
    def search(state, depth):
        if depth > 12:
            return None
        for v in range(256):
            nxt = _literal(state, v)
            a, b = (bytes(x[:len(want)]) for x in _reach(nxt))
            if a.ljust(len(want), b"\x00") == b.ljust(len(want), b"\xff") == want:
                return nxt[3]
            if a.ljust(len(want), b"\x00") <= want <= b.ljust(len(want), b"\xff"):
                got = search(nxt, depth + 1)
                if got:
                    return got
        return None

    for mid in range(a[c] + 1, b[c]):
        want = bytes(a[:c]) + bytes([mid]) + target
        text = search(state, 0)
        if text is not None:
            return prefix, text[len(prefix):], c + 1
    raise AssertionError("no literals give the target")


ACCEPTED = ("distance_equal_to_the_dictionary", "distance_equal_to_the_bytes_written", "length_273_ends_at_data_size", "short_rep_in_front_of_the_marker",
            "every_ds_fraction", "empty_member_between", "header_planted_in_the_payload")
# name -> the decoder's words
REFUSED = {
    "distance_one_beyond_the_dictionary": "member at byte 0: a distance beyond the member's start or dictionary",
    "distance_one_beyond_a_fraction_dictionary": "member at byte 0: a distance beyond the member's start or dictionary",
    "distance_one_beyond_the_bytes_written": "member at byte 0: a distance beyond the member's start or dictionary",
    "short_rep_into_an_empty_dictionary": "member at byte 0: a distance beyond the member's start or dictionary",
    "match_one_byte_over_data_size": "member at byte 0: a match that runs over the member's data_size",
    "marker_one_symbol_early": "member at byte 0: an end marker in front of the member's data_size",
    "text_one_literal_long": "member at byte 0: text that goes on behind the member's data_size",
    "text_one_short_rep_long": "member at byte 0: text that goes on behind the member's data_size",
    "marker_of_length_3": "member at byte 0: a sync-flush marker (length 3) inside a member",
    "marker_of_length_4": "member at byte 0: an end marker of a length other than 2",
    "ds_below_4k": "member at byte 0: a dictionary size below 4 KiB or above 512 MiB",
    "ds_fraction_below_4k": "member at byte 0: a dictionary size below 4 KiB or above 512 MiB",
    "ds_above_512m": "member at byte 0: a dictionary size below 4 KiB or above 512 MiB",
    "first_range_byte_not_zero": "member at byte 0: a range coder that does not start with a zero byte",
    "code_not_zero_at_the_end": "member at byte 0: a range coder that does not end at zero",
    "bytes_between_marker_and_trailer": "member at byte 0: an LZMA stream that does not end at the member's trailer",
}
# what liblzma's raw decoder takes all the same: it ends at a marker of any length (the rule is lzip's own), so of these the
# reference says nothing
REFERENCE_TAKES = ("marker_of_length_3", "marker_of_length_4")


def _co(ops):
    return [lit(b"@CO\t")] + ops + [lit(b"\n")]


_made = {}


def INPUTS(header: bytes, records: bytes):
    """({name: (lzip bytes, text, skip)} that a decoder must take, {name: lzip bytes} that it must refuse with REFUSED[name])."""
    key = (header, records)
    if key in _made:
        return _made[key]
    good, bad = {}, {}
    body = Z.member(header + records, 1 << 16)

    def take(name, *directed):
        """The directed members (blob, text), then the body."""
        text = b"".join(t for _, t in directed)
        good[name] = (b"".join(b for b, _ in directed) + body, text + header + records, len(text) + len(header))

    def refuse(name, blob):
        bad[name] = blob + body

    letters = D._letters
    # the farthest legal distance: exactly the dictionary's size; one more is refused
    take("distance_equal_to_the_dictionary", member_of(_co([lit(letters(4096 - 4, 3)), match(4096, 30)]), 4096))
    refuse("distance_one_beyond_the_dictionary", member_of(_co([lit(letters(4200, 3)), match(4097, 4)]), 4096)[0])
    # a distance equal to the bytes written so far reaches the member's first byte; one more is refused, as is a short rep at byte 0
    take("distance_equal_to_the_bytes_written", member_of(_co([lit(letters(16, 4)), match(20, 20)])))
    refuse("distance_one_beyond_the_bytes_written", member_of(_co([lit(letters(16, 4)), match(21, 4)]))[0])
    refuse("short_rep_into_an_empty_dictionary", member_of([SHORTREP, lit(b"\n")])[0])
    # the longest match ends exactly at data_size: the marker stands right behind it
    line = b"@CO\t" + letters(272, 5) + b"\n"
    take("length_273_ends_at_data_size", member_of([lit(line), lit(b"@CO\t"), match(len(line), 273)]))
    # ... and one byte over it (the trailer states one byte less than the parse writes)
    blob, text = member_of([lit(b"@CO\tabc\n"), match(8, 9)])
    refuse("match_one_byte_over_data_size", member_of([lit(b"@CO\tabc\n"), match(8, 9)], stated=text[:-1])[0])
    # the marker one symbol early, and text one symbol long: a literal, a short rep
    blob, text = member_of(_co([lit(letters(30, 6))]))
    refuse("marker_one_symbol_early", member_of(_co([lit(letters(30, 6))]), stated=text + b"\n")[0])
    refuse("text_one_literal_long", member_of(_co([lit(letters(30, 6))]), stated=text[:-1])[0])
    blob, text = member_of([lit(b"@CO\tq\n"), match(6, 5), SHORTREP])
    take("short_rep_in_front_of_the_marker", (blob, text))
    assert text == b"@CO\tq\n" * 2
    refuse("text_one_short_rep_long", member_of([lit(b"@CO\tq\n"), match(6, 5), SHORTREP], stated=text[:-1])[0])
    # markers of other lengths: 3 is lzlib's sync flush
    for n in (3, 4):
        refuse(f"marker_of_length_{n}", member_of(_co([lit(letters(30, 7))]), marker=match(1 << 32, n))[0])
    # every DS fraction at one base (2^13: all eight are legal), each with a match at its own farthest distance; one more is refused
    fractions = []
    for f in range(8):
        ds = (f << 5) | 13
        d = Z.dict_size_of(ds)
        assert d == 8192 - 512 * f
        fractions.append(member_of(_co([lit(letters(d - 4, 10 + f)), match(d, 11)]), d, ds))
    take("every_ds_fraction", *fractions)
    d = Z.dict_size_of((3 << 5) | 13)
    refuse("distance_one_beyond_a_fraction_dictionary", member_of(_co([lit(letters(d, 13)), match(d + 1, 11)]), d, (3 << 5) | 13)[0])
    small = member_of(_co([lit(letters(30, 8))]))
    refuse("ds_below_4k", Z.MAGIC + b"\x01\x0b" + small[0][6:])
    refuse("ds_fraction_below_4k", Z.MAGIC + b"\x01" + bytes([(1 << 5) | 12]) + small[0][6:])
    refuse("ds_above_512m", Z.MAGIC + b"\x01\x1e" + small[0][6:])
    # an empty member among full ones
    take("empty_member_between", small, (Z.member(b""), b""), member_of(_co([lit(letters(20, 9))])))
    # the range coder's two ends
    refuse("first_range_byte_not_zero", small[0][:6] + b"\x01" + small[0][7:])
    refuse("code_not_zero_at_the_end", small[0][:-21] + bytes([small[0][-21] ^ 1]) + small[0][-20:])
    data, text = stream(_co([lit(letters(30, 8))]))
    refuse("bytes_between_marker_and_trailer", Z.wrap(data + b"\x00", text, Z.ds_byte_of(1 << 16)))
    # a legal header -- LZIP, version 1, a legal DS -- inside the payload, where the finder looks (31 bytes or more into the
    # member): it fails the member_size test and is passed over
    prefix = b"@CO\t" + letters(600, 12)
    target = Z.MAGIC + b"\x01\x0c"
    prefix, planted, off = planted_literals(prefix, target)
    blob, text = member_of([lit(prefix + planted), lit(b"\n")])
    assert blob[6 + off:6 + off + 6] == target and 6 + off >= Z.MEMBER_MIN, (off, blob[6 + off:12 + off])
    take("header_planted_in_the_payload", (blob, text))
    assert tuple(good) != () and set(good) == set(ACCEPTED) and set(bad) == set(REFUSED), (sorted(good), sorted(bad))
    _made[key] = (good, bad)
    return good, bad
