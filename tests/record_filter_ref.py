"""The record filter, restated in Python from its specification (include/slimm_hip.h, "THE RECORD FILTER") -- not a port of
slimm_amd/csrc/record_filter.h: Python integers, regular expressions and struct, one record at a time.  Test infrastructure only.

A filter is a dict with the keys of FILTER_OFF.  A verdict is one of PASS, FLAGS, MAPQ, ALIGNED, IDENTITY, NO_NM, NOT_JUDGED
(the `why` numbers of slimm_host_record_passes_*); `count` turns verdicts into the six counters of
slimm_get_record_filter_stats."""
import re
import struct

PASS, FLAGS, MAPQ, ALIGNED, IDENTITY, NO_NM, NOT_JUDGED = range(7)
STATS = ("judged", "dropped_flags", "dropped_mapq", "dropped_aligned", "dropped_identity", "no_nm")
FILTER_OFF = dict(min_mapq=0, require_flags=0, exclude_flags=0, min_aligned=0, min_identity_permille=0)

_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")
_BAM_OPS = "MIDNSHP=X"


def make(**kw):
    f = dict(FILTER_OFF)
    f.update(kw)
    return f


def dropped(why):
    return why in (FLAGS, MAPQ, ALIGNED, IDENTITY, NO_NM)


def judge(f, flag, mapq, ops, nm):
    """flag, mapq: as they stand in the file; ops: [(length, op letter)] of the CIGAR field ([] for "*"); nm: NM or None."""
    if flag & 0x4:
        return NOT_JUDGED
    if (flag & f["require_flags"]) != f["require_flags"] or (flag & f["exclude_flags"]):
        return FLAGS
    if mapq < f["min_mapq"]:
        return MAPQ
    aligned = sum(n for n, op in ops if op in "M=X")
    columns = sum(n for n, op in ops if op in "M=XID")
    if aligned < f["min_aligned"]:
        return ALIGNED
    permille = f["min_identity_permille"]
    if permille:
        if nm is None:
            return NO_NM
        if not (columns > 0 and 0 <= nm <= columns and (columns - nm) * 1000 >= permille * columns):
            return IDENTITY
    return PASS


def sam_fields(line):
    """(flag, mapq, ops, nm) of one SAM alignment line (str, with or without its newline)."""
    col = line.rstrip("\n").split("\t")
    cigar = col[5]
    ops = [(int(n), op) for n, op in _CIGAR.findall(cigar)] if re.fullmatch(r"(\d+[MIDNSHP=X])+", cigar) else []
    nm = None
    for field in col[11:]:
        if field.startswith("NM:i:"):
            m = re.match(r"[-+]?\d+", field[5:])
            nm = int(m.group()) if m else None
            break
    return int(col[1]) & 0xffff, int(col[4]), ops, nm


def judge_sam(f, line):
    return judge(f, *sam_fields(line))


_SCALAR = {"A": "c", "c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}


def bam_fields(body):
    """(flag, mapq, ops, nm) of one BAM record (bytes behind its block_size word), by the layout of SAM/BAM specification 4.2."""
    l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<BBHHHI", body, 8)
    p = 32 + l_name
    ops = []
    for k in range(n_cigar):
        w = struct.unpack_from("<I", body, p + 4 * k)[0]
        ops.append((w >> 4, _BAM_OPS[w & 15]))
    p += 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    nm = None
    try:
        while p + 3 <= len(body):
            tag, ty = body[p:p + 2], chr(body[p + 2])
            p += 3
            if ty in _SCALAR:
                v = struct.unpack_from("<" + _SCALAR[ty], body, p)[0]
                p += struct.calcsize(_SCALAR[ty])
                if tag == b"NM" and ty in "cCsSiI":
                    nm = v
                    break
            elif ty in "ZH":
                p = body.index(b"\x00", p) + 1
            elif ty == "B":
                sub, n = chr(body[p]), struct.unpack_from("<I", body, p + 1)[0]
                if sub not in "cCsSiIf" or p + 5 + n * struct.calcsize(_SCALAR[sub]) > len(body):
                    break
                p += 5 + n * struct.calcsize(_SCALAR[sub])
            else:
                break   # (a tag area that does not parse: NM absent)
    except (struct.error, ValueError, IndexError):
        nm = None
    return flag, mapq, ops, nm


def judge_bam(f, body):
    return judge(f, *bam_fields(body))


def count(verdicts):
    verdicts = list(verdicts)
    return dict(judged=sum(v != NOT_JUDGED for v in verdicts), dropped_flags=verdicts.count(FLAGS), dropped_mapq=verdicts.count(MAPQ),
                dropped_aligned=verdicts.count(ALIGNED), dropped_identity=verdicts.count(IDENTITY) + verdicts.count(NO_NM),
                no_nm=verdicts.count(NO_NM))


def stats_line(c):
    """The command's log line for these counts."""
    s = (f"record filter: {c['judged']} judged; dropped: {c['dropped_flags']} by flags, {c['dropped_mapq']} by MAPQ, "
         f"{c['dropped_aligned']} by aligned length, {c['dropped_identity']} by identity")
    return s + (f" ({c['no_nm']} of them without NM)" if c["no_nm"] else "")
