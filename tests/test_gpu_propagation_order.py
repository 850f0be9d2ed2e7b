"""The order of the LCA count propagation (Q17) on the device path: the four-contig cases as real records through the
kernels -- one context, the device-side merge of the partial results, and a group of two members on one device --, and a
hole-free stream.  Every integer before the propagation equals the oracle's; the verdict names taxid 0; the profile is
the oracle's under exactly one of the two walks."""
import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import Slimm, SlimmGroup
from slimm_amd.synth import CONFIGS, make_workload
from tests.helpers import assert_matches_oracle, assert_profiles_match
from tests.propagation_cases import FOUR_CONTIG_AB, four_contig_case

pytestmark = pytest.mark.gpu

DEP = capi.PROPAGATION_DEPENDENT


def _before_propagation(s, o):
    """What the device path produced before step 2, with the direct LCA hits held against the oracle's; the rest is held
    against the oracle by tests.helpers.assert_matches_oracle under the walk that is the oracle's, and must be the same
    under the other."""
    assert s.taxon_counts(0) == o.lca_direct, "direct LCA counts differ"
    assert s.children_pairs(0) == o.lca_direct_children, "direct LCA children differ"
    st = s.stats()
    return ({k: v for k, v in st.items() if not k.startswith("profile_")}, {k: v.tolist() for k, v in s.ref_columns().items()},
            s.taxon_counts(0), s.children_pairs(0))


def _equals_oracle(s, o, text=None, bins=True):
    if s.taxon_counts(1) != o.taxon_count or s.children_pairs(1) != o.taxon_children:
        return False
    assert_matches_oracle(s, o, bins=bins)       # every integer, every bin, the profile
    if text is not None:
        assert_profiles_match(text, o.profile_tsv)
    return True


@pytest.fixture(scope="module")
def oracle_of():
    cache = {}

    def get(ab, rank):
        if (ab, rank) not in cache:
            w = four_contig_case(*ab, rank=rank)
            cache[(ab, rank)] = (w, run_workload(w))
        return cache[(ab, rank)]
    return get


@pytest.mark.parametrize("rank", ["species", "family"])
@pytest.mark.parametrize("ab", FOUR_CONTIG_AB)
def test_four_contigs_through_the_kernels(ab, rank, oracle_of):
    w, o = oracle_of(ab, rank)
    s = Slimm.for_workload(w, device=0)
    equal, before = {}, {}
    for walk in (capi.WALK_DEFAULT, capi.WALK_REVERSED):
        s.reset()                                 # (the walk is a setting: it survives)
        s.set_propagation_walk(walk)
        s.push_records(w.records)
        assert s.get_profiles() is not None
        before[walk] = _before_propagation(s, o)
        assert s.propagation_order() == (DEP, [0])
        equal[walk] = _equals_oracle(s, o)
    assert sorted(equal.values()) == [False, True], equal
    assert before[capi.WALK_DEFAULT] == before[capi.WALK_REVERSED]
    s.close()


def test_four_contigs_through_the_device_side_merge(oracle_of):
    """slimm_partials_buffer -> slimm_install_merged_partials (the multi-rank path with one rank: nothing to sum)."""
    w, o = oracle_of((2, 3), "species")
    s = Slimm.for_workload(w, device=0)
    s.set_propagation_walk(capi.WALK_REVERSED)
    s.push_records(w.records)
    s.analyze_alignments()
    assert s.finish_coverage()
    s.filter_alignments()
    s.partials_tensor()
    assert s.install_merged_partials() is not None
    s.get_reads_lca_count()
    before = _before_propagation(s, o)
    assert s.propagation_order() == (DEP, [0])
    one = Slimm.for_workload(w, device=0)
    one.set_propagation_walk(capi.WALK_REVERSED)
    one.push_records(w.records)
    assert one.get_profiles() is not None
    assert before == _before_propagation(one, o)
    assert (s.taxon_counts(1), s.children_pairs(1)) == (one.taxon_counts(1), one.children_pairs(1))
    s.close()
    one.close()


@pytest.mark.parametrize("ab", [(1, 1), (7, 4)])
def test_four_contigs_through_a_group_of_two(ab, oracle_of, tmp_path):
    w, o = oracle_of(ab, "species")
    texts, equal = {}, {}
    for walk in (capi.WALK_DEFAULT, capi.WALK_REVERSED):
        g = SlimmGroup(w, [0, 0])
        g.set_propagation_walk(walk)
        g.push_records(w.records, batch=11)      # (stretches of 11 records: both members hold reads)
        path = str(tmp_path / f"p{walk}.tsv")
        assert g.get_profiles(path)
        m = g.member(0)
        _before_propagation(m, o)
        assert g.propagation_order() == (DEP, [0])
        texts[walk] = open(path).read()
        equal[walk] = _equals_oracle(m, o, texts[walk], bins=False)   # (the coverage arrays stay per-member sums)
        one = Slimm.for_workload(w, device=0)    # the same walk on one context: the same counts, the same text
        one.set_propagation_walk(walk)
        one.push_records(w.records)
        assert one.get_profiles() == texts[walk]
        assert (m.taxon_counts(1), m.children_pairs(1)) == (one.taxon_counts(1), one.children_pairs(1))
        one.close()
        g.close()
    assert sorted(equal.values()) == [False, True], equal
    assert texts[capi.WALK_DEFAULT] != texts[capi.WALK_REVERSED]


def test_hole_free_stream_is_independent_on_the_device():
    w = make_workload(CONFIGS["config1"], seed=2)
    s = Slimm.for_workload(w, device=0)
    s.push_records(w.records)
    assert s.get_profiles() is not None
    assert s.propagation_order() == (capi.PROPAGATION_INDEPENDENT, [])
    assert_matches_oracle(s, run_workload(w), bins=False)
    s.close()
