"""A bzip2 decoder in plain Python that counts the paths an input takes, written from the format as
slimm_amd/csrc/bzip2_block.h's header comment states it: decode(blob) -> (text, Counter of named paths), all_paths() the
names there are, Bad what it raises on a stream it refuses.  tests/bzip2_directed.py writes inputs for chosen paths;
tests/test_codec_paths_bzip2_deflate.py holds both against bz2.decompress.  Test infrastructure only."""
from collections import Counter

import numpy as np

BLOCK_MAGIC, EOS_MAGIC = 0x314159265359, 0x177245385090
MAX_SELECTORS = 18002
RUN_WEIGHTS = 20    # RUNA / RUNB digits of weight 2^0 .. 2^19: a digit of weight 2^20 is refused


class Bad(Exception):
    pass


def all_paths():
    p = [f"level:{k}" for k in range(1, 10)] + ["streams:1", "streams:many", "stream:empty"]
    p += ["orig:0", "orig:n-1", "orig:ruler", "orig:off_ruler", "map:groups:1", "map:groups:16", "used:1", "used:256"]
    p += [f"tables:{k}" for k in range(2, 7)] + ["table:unselected"] + [f"sel_mtf:{k}" for k in range(6)]
    p += ["n_sel:exact", "n_sel:surplus", "n_sel:above_18002"]
    p += ["len_start:1", "len_start:20", "len_step:up", "len_step:down", "len_step:both_in_one_symbol", "len_used:1", "len_used:20", "len:min_eq_max"]
    p += [f"ext:{k}" for k in range(20)]
    p += [f"run{d}:w{k}" for d in "ab" for k in range(RUN_WEIGHTS)]
    p += ["run:at_block_start", "run:before_eob", "run:len:1", "run:len:2", "run:len:3", "run:ends_at_level_limit"]
    p += ["mtf:1", "mtf:255", "eob:first_of_group", "eob:50th_of_group", "n:1", "n:255", "n:256", "n:257", "n:level_limit"]
    p += ["bwt:cycles:1", "bwt:cycles:2", "bwt:cycles:3", "bwt:period:1", "bwt:period:2"]
    p += [f"rle1:count:{k}" for k in (0, 1, 251, 252, 253, 254, 255)] + ["rle1:byte_behind_count_is_the_runs"]
    p += [f"rle1:block_ends_in:{k}:next_begins_same" for k in (1, 2, 3)] + ["rle1:block_ends_in_4_and_count"]
    return p


_CRC = []
for _i in range(256):
    _c = _i << 24
    for _ in range(8):
        _c = ((_c << 1) ^ 0x04c11db7) & 0xffffffff if _c & 0x80000000 else (_c << 1) & 0xffffffff
    _CRC.append(_c)


def crc32_bzip2(data: bytes) -> int:
    """CRC-32, MSB first, polynomial 0x04c11db7 (not zlib's reflected one)."""
    c = 0xffffffff
    for b in data:
        c = ((c << 8) & 0xffffffff) ^ _CRC[(c >> 24) ^ b]
    return c ^ 0xffffffff


class _Reader:
    def __init__(self, blob):
        self.bits = (np.unpackbits(np.frombuffer(blob, dtype=np.uint8)) + 48).astype(np.uint8).tobytes().decode("ascii")
        self.pos = 0

    def get(self, k):
        if self.pos + k > len(self.bits):
            raise Bad("truncated")
        v = int(self.bits[self.pos:self.pos + k], 2) if k else 0
        self.pos += k
        return v


def _block(r, level, c, carry):
    """One block behind its magic: its text.  carry: [trailing equal bytes 1..3 of the block in front, that byte] or None."""
    crc = r.get(32)
    if r.get(1):
        raise Bad("randomised")
    orig = r.get(24)
    used16, used = r.get(16), []
    for i in range(16):
        if used16 >> (15 - i) & 1:
            w = r.get(16)
            used += [16 * i + j for j in range(16) if w >> (15 - j) & 1]
    if not used:
        raise Bad("no byte in use")
    c[f"map:groups:{bin(used16).count('1')}"] += 1
    c[f"used:{len(used)}"] += 1
    alpha = len(used) + 2
    nt, ns = r.get(3), r.get(15)
    if not 2 <= nt <= 6:
        raise Bad("number of tables")
    if ns < 1:
        raise Bad("no selectors")
    c[f"tables:{nt}"] += 1
    order, sels = list(range(nt)), []
    for _ in range(ns):
        j = 0
        while r.get(1):
            j += 1
            if j >= nt:
                raise Bad("selector past the tables")
        order.insert(0, order.pop(j))
        c[f"sel_mtf:{j}"] += 1
        sels.append(order[0])
    for t in range(nt):
        if t not in sels:
            c["table:unselected"] += 1
    tables = []
    for t in range(nt):
        cur, lens = r.get(5), []
        c[f"len_start:{cur}"] += 1
        for _ in range(alpha):
            up = down = 0
            while True:
                if not 1 <= cur <= 20:
                    raise Bad("code length")
                if not r.get(1):
                    break
                if r.get(1):
                    cur, down = cur - 1, down + 1
                else:
                    cur, up = cur + 1, up + 1
            c["len_step:up"] += up > 0
            c["len_step:down"] += down > 0
            c["len_step:both_in_one_symbol"] += up > 0 and down > 0
            lens.append(cur)
        for ln in set(lens):
            c[f"len_used:{ln}"] += 1
        lo, hi = min(lens), max(lens)
        c["len:min_eq_max"] += lo == hi
        code, codes = 0, {}
        for ln in range(lo, hi + 1):   # the canonical code: by length, then by symbol
            for s in range(alpha):
                if lens[s] == ln:
                    codes[format(code, "0%db" % ln)] = s
                    code += 1
            code <<= 1
        tables.append((lo, codes))
    # the symbols
    limit = level * 100_000
    mtf, ll = list(range(len(used))), bytearray()
    run, digit, k, eob = 0, 0, 0, len(used) + 1
    run_from_start = False
    bits = r.bits
    while True:
        if k % 50 == 0:
            if k // 50 >= min(ns, MAX_SELECTORS):
                raise Bad("symbols beyond the selectors")
            lo, codes = tables[sels[k // 50]]
        for ln in range(lo, 21):
            sym = codes.get(bits[r.pos:r.pos + ln])
            if sym is not None:
                break
        else:
            raise Bad("truncated" if r.pos + 20 > len(bits) else "no code")
        if r.pos + ln > len(bits):
            raise Bad("truncated")
        r.pos += ln
        c[f"ext:{ln - lo}"] += 1
        k += 1
        if sym <= 1:
            if digit >= RUN_WEIGHTS:
                raise Bad("run digit of weight 2^20")
            if digit == 0:
                run_from_start = not ll
            run += (1 + sym) << digit
            c[f"run{'ab'[sym]}:w{digit}"] += 1
            digit += 1
            continue
        if run:
            if len(ll) + run > limit:
                raise Bad("run overshoots the block")
            ll += bytes([used[mtf[0]]]) * run
            c[f"run:len:{run}"] += 1
            c["run:at_block_start"] += run_from_start
            c["run:before_eob"] += sym == eob
            c["run:ends_at_level_limit"] += len(ll) == limit
            run = digit = 0
        if sym == eob:
            c["eob:first_of_group"] += k % 50 == 1
            c["eob:50th_of_group"] += k % 50 == 0
            break
        if len(ll) >= limit:
            raise Bad("block longer than its level")
        c[f"mtf:{sym - 1}"] += 1
        mtf.insert(0, mtf.pop(sym - 1))
        ll.append(used[mtf[0]])
    needed = (k + 49) // 50
    c["n_sel:above_18002" if ns > MAX_SELECTORS else "n_sel:surplus" if ns > needed else "n_sel:exact"] += 1
    n = len(ll)
    if orig >= n:
        raise Bad("origPtr")
    c[f"n:{n}"] += 1
    c["n:level_limit"] += n == limit
    c["orig:0"] += orig == 0
    c["orig:n-1"] += orig == n - 1
    c["orig:ruler"] += orig > 0 and orig % 256 == 0
    c["orig:off_ruler"] += orig % 256 != 0
    # the inverse BWT: a counting sort gives each sorted position its successor; n steps from origPtr
    cf, s = [0] * 256, 0
    hist = Counter(ll)
    for b in range(256):
        cf[b], s = s, s + hist[b]
    link = [0] * n
    for i, b in enumerate(ll):
        link[cf[b]] = i
        cf[b] += 1
    rle, p = bytearray(n), orig
    period = 0
    for i in range(n):
        p = link[p]
        rle[i] = ll[p]
        if not period and p == orig:   # (the cycle through origPtr closes: a text that repeats itself goes round it again)
            period = i + 1
    c[f"bwt:cycles:{n // period}"] += 1
    c[f"bwt:period:{period}"] += 1
    # RLE1 undone
    text, last, eq, after_count = bytearray(), -1, 0, False
    if carry and rle[0] == carry[1]:
        c[f"rle1:block_ends_in:{carry[0]}:next_begins_same"] += 1
    for b in rle:
        if eq == 4:
            c[f"rle1:count:{b}"] += 1
            text += bytes([last]) * b
            after_count, eq, prev, last = True, 0, last, -1
            continue
        if after_count:
            c["rle1:byte_behind_count_is_the_runs"] += b == prev
            after_count = False
        eq = eq + 1 if b == last else 1
        last = b
        text.append(b)
    if eq == 4:
        raise Bad("four equal bytes end the block and no count byte follows")
    c["rle1:block_ends_in_4_and_count"] += eq == 0
    if crc32_bzip2(text) != crc:
        raise Bad("block CRC")
    return bytes(text), crc, ([eq, last] if eq else None)


def decode(blob: bytes):
    r, c, out, streams = _Reader(blob), Counter(), [], 0
    carry = None
    while True:
        if r.pos == len(r.bits) and streams:
            break
        if r.get(24) != 0x425a68:
            raise Bad("no stream header")
        level = r.get(8) - 48
        if not 1 <= level <= 9:
            raise Bad("level")
        streams += 1
        c[f"level:{level}"] += 1
        combined, blocks = 0, 0
        while True:
            magic = r.get(48)
            if magic == EOS_MAGIC:
                if r.get(32) != combined:
                    raise Bad("combined CRC")
                r.pos = (r.pos + 7) & ~7
                c["stream:empty"] += blocks == 0
                break
            if magic != BLOCK_MAGIC:
                raise Bad("no block or end-of-stream magic")
            text, crc, carry = _block(r, level, c, carry)
            out.append(text)
            combined = (((combined << 1) | (combined >> 31)) & 0xffffffff) ^ crc
            blocks += 1
            c["count:blocks"] += 1
    c["count:streams"] = streams
    c["streams:1" if streams == 1 else "streams:many"] += 1
    return b"".join(out), +c
