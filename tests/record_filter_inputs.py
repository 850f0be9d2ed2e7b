"""Inputs for the record filter's tests: the files of tests/bam_io.py with MAPQ, CIGAR and tags set per record.

The writers themselves stay as they are: their SAM lines and BAM records are taken apart here and put together again with
the three things they write the same for every record.  Read names do not end in ".1" / ".2" and the read length is constant,
so a copy of a file WITHOUT its dropped records has the file's average read length and its Q18 verdict.  Test infrastructure
only."""
import random
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from slimm_amd.synth import SynthConfig, make_workload
from slimm_amd.workload import Records, Workload
from tests import record_filter_ref as R
from tests.bam_io import _bgzf_block, bam_header_bytes, bam_record_bytes, sam_header, write_sam

READ_LEN = 100
CONFIG = SynthConfig("record-filter", 4_000, 8, 1.8, bin_width=100, len_lo=5_000, len_hi=50_000, present_frac=0.8)
_OPS = "MIDNSHP=X"
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


@dataclass
class Attr:
    """What one record carries besides the four fields of the hot path.  tags: (name, type, value) in file order; an NM of
    type c C s S i I is written as that type in BAM and as NM:i in SAM; Z and H values are str, B values (subtype, [numbers])."""
    mapq: int = 255
    cigar: Optional[List[Tuple[int, str]]] = None   # None: "*"
    tags: list = field(default_factory=list)


def sam_tag(t):
    name, ty, v = t
    if ty in _INT:
        return f"{name}:i:{v}"
    if ty == "B":
        return f"{name}:B:{v[0]}," + ",".join(str(x) for x in v[1])
    return f"{name}:{ty}:{v}"


def bam_tag(t):
    name, ty, v = t
    if ty in _INT:
        return name.encode() + ty.encode() + struct.pack(_INT[ty], v)
    if ty == "A":
        return name.encode() + b"A" + v.encode()
    if ty == "f":
        return name.encode() + b"f" + struct.pack("<f", v)
    if ty == "B":
        return name.encode() + b"B" + v[0].encode() + struct.pack("<I", len(v[1])) + b"".join(struct.pack(_INT[v[0]], x) for x in v[1])
    return name.encode() + ty.encode() + v.encode() + b"\x00"


def cigar_text(ops):
    return "".join(f"{n}{op}" for n, op in ops) if ops else "*"


def sam_lines(w: Workload, attrs, tmp_path) -> List[str]:
    """The alignment lines of write_sam's file (no header), fields 5, 6 and 12.. replaced."""
    p = str(tmp_path / "rf_plain.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=READ_LEN)
    lines = [ln for ln in open(p).read().split("\n") if ln and not ln.startswith("@")]
    assert len(lines) == len(attrs)
    out = []
    for ln, a in zip(lines, attrs):
        col = ln.split("\t")[:11]
        col[4], col[5] = str(a.mapq), cigar_text(a.cigar)
        out.append("\t".join(col + [sam_tag(t) for t in a.tags]))
    return out


def sam_file_text(w: Workload, lines, tail_newline=True) -> bytes:
    body = "\n".join(lines) + ("\n" if tail_newline else "")
    return (sam_header(w.ref_names, w.ref_len) + body).encode()


def bam_bodies(w: Workload, attrs) -> List[bytes]:
    """The records of bam_record_bytes (each behind its block_size word), MAPQ, CIGAR and tags replaced."""
    data = bam_record_bytes(w.records, read_len=READ_LEN)
    out, p = [], 0
    for a in attrs:
        bs = struct.unpack_from("<i", data, p)[0]
        body = data[p + 4:p + 4 + bs]
        p += 4 + bs
        l_name, _mapq, bin_, n_cigar, flag, l_seq = struct.unpack_from("<BBHHHI", body, 8)
        name_end = 32 + l_name
        seq_qual = body[name_end + 4 * n_cigar:name_end + 4 * n_cigar + (l_seq + 1) // 2 + l_seq]
        ops = a.cigar or []
        cg = b"".join(struct.pack("<I", (n << 4) | _OPS.index(op)) for n, op in ops)
        head = body[:8] + struct.pack("<BBHHHI", l_name, a.mapq, bin_, len(ops), flag, l_seq) + body[20:name_end]
        out.append(head + cg + seq_qual + b"".join(bam_tag(t) for t in a.tags))
    assert p == len(data)
    return out


def bam_bytes(bodies) -> bytes:
    return b"".join(struct.pack("<i", len(b)) + b for b in bodies)


def bam_file(path, w: Workload, bodies, block=0xff00):
    out = bam_header_bytes(w.ref_names, w.ref_len) + bam_bytes(bodies)
    with open(path, "wb") as f:
        for s in range(0, len(out), block):
            f.write(_bgzf_block(out[s:s + block]))
        f.write(_bgzf_block(b""))


def bgzf_of(data: bytes, seed: int, lo=500, hi=65_000) -> bytes:
    """`data` in BGZF blocks cut at random places, with the end-of-file block."""
    rng, p, out = random.Random(seed), 0, []
    while p < len(data):
        n = rng.randint(lo, hi)
        out.append(_bgzf_block(data[p:p + n]))
        p += n
    return b"".join(out) + _bgzf_block(b"")


def named(w: Workload) -> Workload:
    r = w.records
    ids = np.unique(r.read_key, return_inverse=True)[1]
    names = ["read/%d/" % i for i in ids.tolist()]
    return Workload(w.ref_names, w.ref_len, w.taxonomy, Records(r.read_key, r.flag, r.ref_id, r.begin_pos, names), w.avg_read_len,
                    w.options, w.name + "-named", grouped=w.grouped)


def subset(w: Workload, keep) -> Workload:
    idx = np.nonzero(np.asarray(keep))[0]
    r = w.records
    rec = Records(r.read_key[idx], r.flag[idx], r.ref_id[idx], r.begin_pos[idx], [r.qname[i] for i in idx.tolist()])
    return Workload(w.ref_names, w.ref_len, w.taxonomy, rec, w.avg_read_len, w.options, w.name + "-kept", grouped=w.grouped)


def _many_ops(rng):
    """40 operations over READ_LEN query bases: M runs with single-base insertions and deletions between them."""
    ops, left = [], READ_LEN
    for k in range(20):
        last = k == 19
        m = left if last else rng.randint(2, max(2, left // (20 - k) - 1))
        ops.append((m, "M" if k % 5 else "="))
        left -= m
        if last:
            ops.append((3, "H"))
        elif k % 2:
            ops.append((1, "I"))
            left -= 1
        else:
            ops.append((1, "D"))
    assert len(ops) == 40
    return ops


def _attr(rng) -> Attr:
    u = rng.random()
    if u < 0.55:
        cigar = [(READ_LEN, "M")]
    elif u < 0.67:
        cigar = [(40, "M"), (2, "I"), (30, "M"), (3, "D"), (28, "X")]
    elif u < 0.77:
        cigar = _many_ops(rng)
    elif u < 0.95:
        s = rng.randint(55, 80)
        cigar = [(s, "S"), (READ_LEN - s, "M")]
    elif u < 0.98:
        cigar = None
    else:
        cigar = [(20, "H"), (READ_LEN, "S")]
    mapq = rng.choice([0, 1, 3, 9]) if rng.random() < 0.3 else rng.choice([10, 11, 30, 42, 60, 60, 60, 255])
    tags = []
    if rng.random() < 0.6:
        tags.append(("MD", "Z", "".join(rng.choice("ACGT0123456789^") for _ in range(rng.randint(1, 40)))))
    if rng.random() < 0.15:   # a long tag area in front of NM
        tags.append(("XA", "Z", ";".join("chr%d,+%d,100M,%d" % (rng.randint(1, 22), rng.randint(1, 10 ** 8), rng.randint(0, 9)) for _ in range(12))))
    if rng.random() < 0.2:
        tags.append(("XH", "H", "%08X" % rng.getrandbits(32)))
    if rng.random() < 0.2:
        tags.append(("XB", "B", ("i", [rng.randint(-999, 999) for _ in range(rng.randint(0, 30))])))
    if rng.random() < 0.94:
        nm = rng.randint(0, 4) if rng.random() < 0.65 else rng.randint(6, 15)
        at = rng.randint(0, len(tags))
        tags.insert(at, ("NM", "C" if nm > 127 else rng.choice("cCsSiI"), nm))
    if rng.random() < 0.3:
        tags.append(("AS", "i", rng.randint(0, 200)))
    return Attr(mapq, cigar, tags)


FILTERS = {   # each option of the command alone, and all of them together
    "mapq": R.make(min_mapq=10),
    "require": R.make(require_flags=0x2),
    "exclude": R.make(exclude_flags=0xE00),
    "aligned": R.make(min_aligned=50),
    "identity": R.make(min_identity_permille=950),
    "all": R.make(min_mapq=10, require_flags=0x2, exclude_flags=0xE00, min_aligned=50, min_identity_permille=950),
}


def workload_and_attrs(grouped: bool, seed: int = 7):
    """About 4 000 records over 8 references, read names kept, with flags 0x2 / 0x200 / 0x400 / 0x800 dealt at random; one
    reference's records all get MAPQ 0 (the reference loses all its reads under -q)."""
    w = named(make_workload(CONFIG, seed=seed, shuffled=not grouped))
    rng = random.Random(seed)
    r = w.records
    attrs = [_attr(rng) for _ in range(len(r))]
    flag = r.flag.copy()
    for i in range(len(r)):
        if rng.random() < 0.75:
            flag[i] |= 0x2
        if rng.random() < 0.2:
            flag[i] |= rng.choice([0x200, 0x400, 0x800])
    r.flag[:] = flag
    mapped = r.ref_id[(r.flag & 4) == 0]
    ids, n = np.unique(mapped[mapped >= 0], return_counts=True)
    lost = int(ids[np.argsort(n)[len(n) // 2]])
    for i in np.nonzero(r.ref_id == lost)[0].tolist():
        attrs[i].mapq = 0
    return w, attrs, lost


def input_conditions(w: Workload, verdicts_by_filter):
    """What keeps a filter that does nothing from passing: asserted from the Python restatement's verdicts."""
    r = w.records
    n = len(r)
    for name, v in verdicts_by_filter.items():
        if name == "all":
            continue
        judged = sum(x != R.NOT_JUDGED for x in v)
        share = sum(R.dropped(x) for x in v) / judged
        assert 0.10 <= share <= 0.60, (name, share)
    v = verdicts_by_filter["all"]
    before, after = {}, {}
    for i in range(n):
        if (int(r.flag[i]) & 4) or int(r.ref_id[i]) < 0:
            continue
        key = (r.qname[i], int(r.flag[i]) & 0xC0)
        before.setdefault(key, set()).add(int(r.ref_id[i]))
        if not R.dropped(v[i]):
            after.setdefault(key, set()).add(int(r.ref_id[i]))
    assert any(k not in after for k in before), "no read loses all its alignments"
    assert any(len(before[k]) > 1 and len(after[k]) == 1 for k in after), "no read goes from several references to one"
    refs_before = set().union(*before.values())
    refs_after = set().union(*after.values())
    assert refs_before - refs_after, "no reference loses all its reads"
