"""The stable partition of records by owner, by itself (slimm_amd/csrc/deal_by_key.hip; include/slimm_hip.h:
slimm_partition_by_key) against numpy's stable sort by owner: how a group deals a file in any order to its members on the
device.  owner = (key & (2^62 - 1)) % m, the rule of the host dealing (group.hip: deal); the order inside a stretch is the
input order.  All five arrays and the stretch lengths must be equal."""
import os
import re

import numpy as np
import pytest

from slimm_amd import capi
from slimm_amd.profiler import partition_by_key

pytestmark = pytest.mark.gpu

KEY_MASK = (1 << 62) - 1


def _constants():
    """kDealGrid and the records of a round, as the code has them."""
    src = open(os.path.join(os.path.dirname(capi.__file__), "csrc", "deal_by_key.h")).read()
    grid = int(re.search(r"constexpr uint32_t kDealGrid = (\d+);", src).group(1))
    items = int(re.search(r"constexpr uint32_t kDealItems = (\d+);", src).group(1))
    assert re.search(r"constexpr uint32_t kDealRound = 64 \* kDealItems;", src)
    return grid, 64 * items


GRID, ROUND = _constants()


def stretch(n: int) -> int:
    """deal_stretch: the records of one workgroup's stretch, whole rounds."""
    per = (n + GRID - 1) // GRID
    return (per + ROUND - 1) // ROUND * ROUND


# up to GRID * ROUND records a stretch is one round: fewer than, exactly and one more than a stretch, several stretches;
# every one of them leaves trailing workgroups without records.  LARGE: two rounds per stretch, about half the workgroups idle
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, ROUND - 1, ROUND, ROUND + 1, 5 * ROUND + 3]
LARGE = GRID * ROUND + 1
MEMBERS = [1, 2, 3, 7, 16, 255]
KINDS = ["top_bits", "same", "iota", "random62"]


def keys_of(kind: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(n * 7 + len(kind))
    if kind == "top_bits":   # bits 62 and 63 set: they are not part of the identity
        return rng.integers(0, 1 << 62, n, dtype=np.uint64) | np.uint64(3 << 62)
    if kind == "same":       # one owner takes all
        return np.full(n, 0x123456789abcdef, dtype=np.uint64)
    if kind == "iota":
        return np.arange(n, dtype=np.uint64)
    return rng.integers(0, 1 << 62, n, dtype=np.uint64)


def columns(n: int):
    """(ref, pos, flag, check): functions of the index, so that a misplaced lane shows"""
    i = np.arange(n, dtype=np.uint64)
    check = ((i * np.uint64(0x9e3779b97f4a7c15)) >> np.uint64(32)).astype(np.uint32)
    return (i % np.uint64(1000)).astype(np.int32), i.astype(np.int32), (i % np.uint64(65536)).astype(np.uint16), check


def check_partition(key, m, with_check=True):
    n = len(key)
    ref, pos, flag, check = columns(n)
    owner = ((key & np.uint64(KEY_MASK)) % np.uint64(m)).astype(np.int64)
    order = np.argsort(owner, kind="stable")
    got = partition_by_key(key, ref, pos, flag, check if with_check else None, m)
    assert np.array_equal(got[5], np.bincount(owner, minlength=m).astype(np.uint64))
    assert np.array_equal(got[1], ref[order]), "ref"
    assert np.array_equal(got[2], pos[order]), "pos (the input index)"
    assert np.array_equal(got[0], key[order]), "key"
    assert np.array_equal(got[3], flag[order]), "flag"
    if with_check:
        assert np.array_equal(got[4], check[order]), "check"
    else:
        assert got[4] is None


def test_the_stretch_is_one_round_for_the_small_sizes():
    assert all(stretch(n) == ROUND for n in SIZES if n) and stretch(LARGE) == 2 * ROUND
    assert -(-LARGE // stretch(LARGE)) < GRID   # (trailing workgroups without records)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", MEMBERS)
def test_partition_equals_a_stable_sort_by_owner(m, kind):
    for n in SIZES:
        check_partition(keys_of(kind, n), m)


@pytest.mark.parametrize("m", [3, 255])
def test_partition_without_check_words(m):
    for n in (0, 65, 5 * ROUND + 3):
        check_partition(keys_of("random62", n), m, with_check=False)


@pytest.mark.parametrize("m,kind", [(3, "random62"), (255, "top_bits"), (7, "same")])
def test_partition_with_longer_stretches_and_idle_workgroups(m, kind):
    check_partition(keys_of(kind, LARGE), m)


def test_partition_refuses_bad_member_counts():
    for m in (0, 256):
        with pytest.raises(capi.SlimmError):
            partition_by_key(np.zeros(4, np.uint64), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint16), None, m)
