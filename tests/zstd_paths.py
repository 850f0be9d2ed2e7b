"""A path-counting zstd decoder in plain Python, written from RFC 8878 -- not from slimm_amd/csrc/zstd_frame.h or the
kernels --: the frames of a file to their bytes and a Counter of the named paths they took (block types, literals forms,
Huffman descriptions, table modes, FSE descriptions, the three codes' values, the kinds of offset and what a repeated offset
was made from, what a match reaches).  By it tests state which paths of the entropy decoders an input reaches.  Slow; test
infrastructure only."""
import struct
from collections import Counter

from tests.sam_zst import xxh64

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEFAULT = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_DEFAULT = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)
TABLES = ("ll", "of", "ml")
MODES = ("predefined", "rle", "fse", "repeat")
MAX_LOG = {"ll": 9, "of": 8, "ml": 9, "weights": 6}
MAX_SYMBOL = {"ll": 35, "of": 31, "ml": 52, "weights": 255}
BLOCK_TYPES = ("raw", "rle", "compressed")


class Bad(Exception):
    pass


def read_fse_description(b, at, end, name, paths):
    """The normalised counts of the description at b[at:end): (counts, accuracy log, the bytes it takes)."""
    bit = at * 8

    def get(k):
        nonlocal bit
        if (bit + k + 7) // 8 > end:
            raise Bad("FSE description runs out")
        v = (int.from_bytes(b[bit >> 3:(bit >> 3) + 4], "little") >> (bit & 7)) & ((1 << k) - 1)
        bit += k
        return v

    log = get(4) + 5
    if log > MAX_LOG[name]:
        raise Bad("FSE accuracy log above the table's maximum")
    paths[f"fse:{name}:al{log}"] += 1
    remaining, counts = 1 << log, []
    while remaining > 0:
        bits = (remaining + 1).bit_length()
        val = get(bits)
        lower = (1 << (bits - 1)) - 1
        threshold = (1 << bits) - 1 - (remaining + 1)
        if (val & lower) < threshold:
            bit -= 1
            val &= lower
        elif val > lower:
            val -= threshold
        p = val - 1
        if p < 0:
            paths[f"fse:{name}:less_than_1"] += 1
        remaining -= 1 if p < 0 else p
        counts.append(p)
        if p == 0:
            flags = 0
            while True:
                r = get(2)
                counts += [0] * r
                flags += 1
                if r != 3:
                    break
            paths[f"fse:{name}:zero_repeat"] += 1
            if flags > 1:
                paths[f"fse:{name}:zero_repeat_chain"] += 1
    if remaining < 0 or len(counts) > MAX_SYMBOL[name] + 1:
        raise Bad("bad FSE description")
    return counts, log, (bit + 7) // 8 - at


def fse_table(counts, log):
    """[(symbol, bits, baseline)] per state."""
    size = 1 << log
    sym, high = [0] * size, size - 1
    nxt = {}
    for s, c in enumerate(counts):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(counts):
        if c > 0:
            nxt[s] = c
            for _ in range(c):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
    if pos:
        raise Bad("bad FSE description")
    out = []
    for i in range(size):
        s = sym[i]
        x = nxt[s]
        nxt[s] = x + 1
        nb = log - (x.bit_length() - 1)
        out.append((s, nb, (x << nb) - size))
    return out


class Backward:
    """A bitstream read from its last byte's padding mark down; bits in front of the first byte are zeros."""
    def __init__(self, b, at, end):
        if end <= at or b[end - 1] == 0:
            raise Bad("a bitstream that does not end on its padding bit")
        self.b, self.at = b, at
        self.pos = (end - at) * 8 - (9 - b[end - 1].bit_length())   # (bits left below the padding mark)

    def read(self, n):
        self.pos -= n
        return self.peek_at(self.pos, n)

    def peek_at(self, lo, n):
        if n == 0:
            return 0
        if lo < 0:
            return self.peek_at(0, n + lo) << -lo if n + lo > 0 else 0
        q = self.at + (lo >> 3)
        return (int.from_bytes(self.b[q:q + 5], "little") >> (lo & 7)) & ((1 << n) - 1)


def huffman_table(weights, paths):
    total = sum(1 << (w - 1) for w in weights if w)
    if total == 0:
        raise Bad("bad Huffman weights")
    max_bits = total.bit_length()
    left = (1 << max_bits) - total
    if left & (left - 1):
        raise Bad("bad Huffman weights")
    weights = weights + [left.bit_length()]
    if max_bits > 11 or len(weights) > 256:
        raise Bad("bad Huffman weights")
    paths[f"huf:maxbits:{max_bits}"] += 1
    table = []
    for w in range(1, max_bits + 1):
        for s, x in enumerate(weights):
            if x == w:
                table += [(s, max_bits + 1 - w)] * (1 << (w - 1))
    return table, max_bits


def read_huffman(b, at, end, paths):
    """The tree description at b[at]: (table, max bits, bytes taken)."""
    h = b[at]
    if h >= 128:
        n = h - 127
        paths["huf:direct"] += 1
        raw = b[at + 1:at + 1 + (n + 1) // 2]
        weights = [(raw[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
        used = 1 + (n + 1) // 2
    else:
        paths["huf:fse"] += 1
        if at + 1 + h > end:
            raise Bad("bad Huffman weights")
        counts, log, took = read_fse_description(b, at + 1, at + 1 + h, "weights", paths)
        t = fse_table(counts, log)
        bs = Backward(b, at + 1 + took, at + 1 + h)
        s1, s2 = bs.read(log), bs.read(log)
        if bs.pos < 0:
            raise Bad("bad Huffman weights")
        weights = []
        while True:
            weights.append(t[s1][0])
            s1 = t[s1][2] + bs.read(t[s1][1])
            if bs.pos < 0:
                weights.append(t[s2][0])
                break
            weights.append(t[s2][0])
            s2 = t[s2][2] + bs.read(t[s2][1])
            if bs.pos < 0:
                weights.append(t[s1][0])
                break
        used = 1 + h
    if any(w > 11 for w in weights):
        raise Bad("bad Huffman weights")
    table, max_bits = huffman_table(weights, paths)
    return table, max_bits, used


def huffman_stream(b, at, end, n, table, max_bits, out):
    bs = Backward(b, at, end)
    mask = (1 << max_bits) - 1
    state = bs.read(max_bits)
    for _ in range(n):
        s, nb = table[state]
        out.append(s)
        state = ((state << nb) | bs.read(nb)) & mask
    if bs.pos != -max_bits:
        raise Bad("literals total disagrees with the block")


class Frame:
    """What lasts over a frame's blocks."""
    def __init__(self, window):
        self.window, self.out, self.reps, self.huf, self.tables = window, bytearray(), [1, 4, 8], None, {}
        self.blocks = []     # (type, end in out) of the blocks so far
        self.sequences = 0          # (of the frame's blocks so far)
        self.no_sequences = False   # (the last block was a compressed one without sequences)


def decode_block(b, at, end, f, paths):
    """One compressed block's bytes b[at:end) onto f.out."""
    b0 = b[at]
    t, fmt = b0 & 3, (b0 >> 2) & 3
    # ---- literals
    if t < 2:
        hb = (1, 2, 1, 3)[fmt]
        regen = int.from_bytes(b[at:at + hb], "little") >> (3 if hb == 1 else 4)
        comp, streams = (regen if t == 0 else 1), 1
    else:
        hb, nb = (3, 3, 4, 5)[fmt], (10, 10, 14, 18)[fmt]
        v = int.from_bytes(b[at:at + hb], "little") >> 4
        regen, comp, streams = v & ((1 << nb) - 1), (v >> nb) & ((1 << nb) - 1), 1 if fmt == 0 else 4
    paths[f"lit:{('raw', 'rle', 'huffman', 'treeless')[t]}:sf{fmt}:streams{streams}"] += 1
    p = at + hb
    if p + comp > end:
        raise Bad("a literals section larger than its block")
    if t == 0:
        lits = b[p:p + regen]
    elif t == 1:
        lits = b[p:p + 1] * regen
    else:
        q = p
        if t == 2:
            table, max_bits, used = read_huffman(b, p, p + comp, paths)
            f.huf = (table, max_bits)
            q += used
        elif f.huf is None:
            raise Bad("treeless literals with no tree in front")
        table, max_bits = f.huf
        lits = bytearray()
        if streams == 1:
            huffman_stream(b, q, p + comp, regen, table, max_bits, lits)
        else:
            s1, s2, s3 = struct.unpack_from("<3H", b, q)
            q += 6
            each = (regen + 3) // 4
            ends = [q + s1, q + s1 + s2, q + s1 + s2 + s3, p + comp]
            if ends[2] >= ends[3] or regen < 3 * each:
                raise Bad("literals total disagrees with the block")
            for k in range(4):
                huffman_stream(b, q if k == 0 else ends[k - 1], ends[k], each if k < 3 else regen - 3 * each, table, max_bits, lits)
    p += comp
    # ---- sequences
    if p >= end:
        raise Bad("sequence total disagrees with the block")
    n0 = b[p]
    if n0 == 0:
        n_seq, p = 0, p + 1
        paths["nseq:0"] += 1
    elif n0 < 128:
        n_seq, p = n0, p + 1
        paths["nseq:1byte"] += 1
    elif n0 < 255:
        n_seq, p = ((n0 - 128) << 8) + b[p + 1], p + 2
        paths["nseq:2byte"] += 1
    else:
        n_seq, p = b[p + 1] + (b[p + 2] << 8) + 0x7F00, p + 3
        paths["nseq:3byte"] += 1
    paths[f"nseq:{n_seq}"] += n_seq in (0, 127, 128, 0x7EFF, 0x7F00)
    reps = [(v, (i, 0)) for i, v in enumerate(f.reps)]   # (value, (the entry slot it came from, times decremented) or None)
    out, lp = f.out, 0
    if n_seq == 0:
        if p != end:
            raise Bad("sequence total disagrees with the block")
    else:
        m = b[p]
        p += 1
        if m & 3:
            raise Bad("a reserved bit is set")
        paths[f"mode_byte:0x{m:02x}"] += 1
        tabs = {}
        for k, name in enumerate(TABLES):
            mode = (m >> (6 - 2 * k)) & 3
            paths[f"mode:{name}:{MODES[mode]}"] += 1
            if mode == 0:
                counts, log = {"ll": LL_DEFAULT, "of": OF_DEFAULT, "ml": ML_DEFAULT}[name]
                f.tables[name] = (fse_table(counts, log), log, "predefined")
            elif mode == 1:
                if b[p] > MAX_SYMBOL[name]:
                    raise Bad("bad sequence code")
                f.tables[name] = ([(b[p], 0, 0)], 0, "rle")
                p += 1
                if n_seq > 1:
                    paths[f"mode:{name}:rle:many_sequences"] += 1
            elif mode == 2:
                counts, log, took = read_fse_description(b, p, end, name, paths)
                f.tables[name] = (fse_table(counts, log), log, "fse")
                p += took
            else:
                if name not in f.tables:
                    raise Bad("a repeated table with none in front to repeat")
                paths[f"mode:{name}:repeat:after_{f.tables[name][2]}"] += 1
            tabs[name] = f.tables[name]
        bs = Backward(b, p, end)
        (lt, ll_log, _), (ot, of_log, _), (mt, ml_log, _) = tabs["ll"], tabs["of"], tabs["ml"]
        ls, os_, ms = bs.read(ll_log), bs.read(of_log), bs.read(ml_log)
        for i in range(n_seq):
            lc, oc, mc = lt[ls][0], ot[os_][0], mt[ms][0]
            if oc > 31:
                raise Bad("bad sequence code")
            oe = bs.read(oc)
            me = bs.read(ML_BITS[mc])
            le = bs.read(LL_BITS[lc])
            paths[f"of_code:{oc}"] += 1
            paths[f"ll_code:{lc}"] += 1
            paths[f"ml_code:{mc}"] += 1
            for name, c, nb, e in (("ll", lc, LL_BITS[lc], le), ("ml", mc, ML_BITS[mc], me), ("of", oc, oc, oe)):
                if nb and e == (1 << nb) - 1:
                    paths[f"{name}_code:{c}:ones"] += 1
                if nb and e == 0:
                    paths[f"{name}_code:{c}:zeros"] += 1
            ll, ml, ofv = LL_BASE[lc] + le, ML_BASE[mc] + me, (1 << oc) + oe
            if ofv > 3:
                reps = [(ofv - 3, None)] + reps[:2]
                paths["of:new"] += 1
            else:
                idx = ofv - 1 + (ll == 0)
                paths[f"of:rep:idx{idx}:{'ll0' if ll == 0 else 'll>0'}"] += 1
                v, origin = reps[min(idx, 2) if idx < 3 else 0]
                paths[f"of:rep:idx{idx}:{'entry' if origin else 'plain'}"] += 1
                if origin:
                    paths[f"of:rep:entry_slot{origin[0]}:decremented{origin[1]}"] += 1
                if i == 0 and not f.sequences:
                    paths[f"of:rep:first_of_frame:idx{idx}"] += 1
                if idx == 1:
                    reps = [reps[1], reps[0], reps[2]]
                elif idx == 2:
                    reps = [reps[2], reps[0], reps[1]]
                elif idx == 3:
                    if v - 1 == 0:
                        raise Bad("a repeated offset minus one that is zero")
                    reps = [(v - 1, (origin[0], origin[1] + 1) if origin else None), reps[0], reps[1]]
            off = reps[0][0]
            if lp + ll > len(lits):
                raise Bad("literals total disagrees with the block")
            out += lits[lp:lp + ll]
            lp += ll
            n = len(out)
            if off > n or off > f.window:
                raise Bad("an offset beyond the frame's start or window")
            if off == n:
                paths["reach:frame_start"] += 1
            if off == f.window:
                paths["reach:window_edge"] += 1
            src = n - off
            for kind, e in f.blocks:
                if e > src:
                    paths[f"reach:earlier_block:{kind}"] += 1
                    break
            if off < ml:
                paths["copy:offset<length"] += 1
                for _ in range(ml):
                    out.append(out[len(out) - off])
            else:
                out += out[src:src + ml]
            if i + 1 < n_seq:
                ls = lt[ls][2] + bs.read(lt[ls][1])
                ms = mt[ms][2] + bs.read(mt[ms][1])
                os_ = ot[os_][2] + bs.read(ot[os_][1])
        if bs.pos != 0:
            raise Bad("sequence total disagrees with the block")
        alive = sum(1 for _, o in reps if o)
        paths[f"exit:entry_slots_alive:{alive}"] += 1
    out += lits[lp:]
    f.sequences += n_seq
    f.reps = [v for v, _ in reps]
    return n_seq


def decode(blob: bytes, check=True):
    """Every frame of a zstd file: (the text, the Counter of paths)."""
    text, paths, p = [], Counter(), 0
    while p < len(blob):
        magic = struct.unpack_from("<I", blob, p)[0]
        if (magic & 0xfffffff0) == 0x184D2A50:
            paths["frame:skippable"] += 1
            p += 8 + struct.unpack_from("<I", blob, p + 4)[0]
            continue
        if magic != 0xFD2FB528:
            raise Bad("bytes behind the last frame that start no frame")
        d = blob[p + 4]
        q = p + 5
        single, fcs = (d >> 5) & 1, d >> 6
        if d & 0x08:
            raise Bad("a reserved bit is set")
        if d & 3:
            raise Bad("a dictionary is needed")
        window = None
        if not single:
            w = blob[q]
            q += 1
            window = (1 << (10 + (w >> 3))) + ((1 << (10 + (w >> 3))) >> 3) * (w & 7)
        nf = (single, 2, 4, 8)[fcs]
        size = None
        if nf:
            size = int.from_bytes(blob[q:q + nf], "little") + (256 if nf == 2 else 0)
            q += nf
        f = Frame(window if window is not None else size)
        paths["frame"] += 1
        while True:
            h = int.from_bytes(blob[q:q + 3], "little")
            last, kind, n = h & 1, (h >> 1) & 3, h >> 3
            q += 3
            if kind == 3:
                raise Bad("reserved block type")
            paths[f"block:{'later' if f.blocks else 'first'}:{BLOCK_TYPES[kind]}"] += 1
            if f.blocks:
                paths[f"block:{BLOCK_TYPES[kind]}:after_{f.blocks[-1][0]}"] += 1
            if n > min(f.window, 1 << 17) and kind != 2 or kind == 2 and n > 1 << 17:
                raise Bad("a block larger than its maximum")
            if kind == 0:
                f.out += blob[q:q + n]
                q += n
            elif kind == 1:
                f.out += blob[q:q + 1] * n
                q += 1
            else:
                before = list(f.reps)
                n_seq = decode_block(blob, q, q + n, f, paths)
                q += n
                if f.blocks and before != [1, 4, 8] and n_seq:
                    paths["reps:carried_into_compressed_block"] += 1
                    if f.blocks[-1][0] != "compressed":
                        paths[f"reps:carried_over_{f.blocks[-1][0]}_block"] += 1
                    elif f.no_sequences:
                        paths["reps:carried_over_compressed_block_without_sequences"] += 1
            f.no_sequences = kind == 2 and n_seq == 0
            f.blocks.append((BLOCK_TYPES[kind], len(f.out)))
            if last:
                break
        if d & 4:
            if check and struct.unpack_from("<I", blob, q)[0] != xxh64(bytes(f.out)) & 0xffffffff:
                raise Bad("content checksum mismatch")
            paths["frame:checksum"] += 1
            q += 4
        if size is not None and size != len(f.out):
            raise Bad("content size mismatch")
        text.append(bytes(f.out))
        p = q
    return b"".join(text), paths


def all_paths():
    """Every path name the decoder can count on a valid stream, the size-bounded ones included."""
    out = [f"block:{w}:{t}" for w in ("first", "later") for t in BLOCK_TYPES]
    out += [f"lit:{t}:sf{k}:streams1" for t in ("raw", "rle") for k in range(4)]
    out += [f"lit:{t}:sf{k}:streams{1 if k == 0 else 4}" for t in ("huffman", "treeless") for k in range(4)]
    out += ["huf:direct", "huf:fse", "huf:maxbits:11", "fse:weights:al5", "fse:weights:al6"]
    out += [f"mode:{t}:{m}" for t in TABLES for m in MODES] + [f"mode:{t}:repeat:after_{m}" for t in TABLES for m in MODES[:3]]
    out += [f"mode:{t}:rle:many_sequences" for t in TABLES] + [f"mode_byte:0x{m << 2:02x}" for m in range(64)]
    out += [f"fse:{t}:al{k}" for t in TABLES for k in range(5, MAX_LOG[t] + 1)]
    out += [f"fse:{t}:{p}" for t in TABLES for p in ("less_than_1", "zero_repeat", "zero_repeat_chain")]
    out += ["nseq:0", "nseq:1byte", "nseq:2byte", "nseq:3byte", "nseq:127", "nseq:128", f"nseq:{0x7EFF}", f"nseq:{0x7F00}"]
    for name, bits in (("of", list(range(32))), ("ll", LL_BITS), ("ml", ML_BITS)):
        out += [f"{name}_code:{c}" for c in range(len(bits))]
        out += [f"{name}_code:{c}:{e}" for c, nb in enumerate(bits) if nb and not (name == "of" and c < 2) for e in ("zeros", "ones")]
    out += ["of:new"] + [f"of:rep:idx{i}:{w}" for i, w in ((0, "ll>0"), (1, "ll0"), (1, "ll>0"), (2, "ll0"), (2, "ll>0"), (3, "ll0"))]
    out += [f"of:rep:idx{i}:{w}" for i in range(4) for w in ("entry", "plain")]
    out += [f"of:rep:entry_slot{i}:decremented{k}" for i in range(3) for k in range(2)] + ["of:rep:entry_slot0:decremented2"]
    out += [f"of:rep:first_of_frame:idx{i}" for i in range(3)] + [f"exit:entry_slots_alive:{n}" for n in range(4)]
    out += ["reps:carried_into_compressed_block", "reps:carried_over_raw_block", "reps:carried_over_rle_block",
            "reps:carried_over_compressed_block_without_sequences"]
    out += [f"reach:earlier_block:{t}" for t in BLOCK_TYPES] + ["reach:frame_start", "reach:window_edge", "copy:offset<length"]
    return out
