"""The order of the LCA count propagation (Q17): the verdict, the taxa involved and the walk setters, on host-only
contexts (device = -1) fed the oracle's integers or hand-made direct hits.  No GPU call is made.

INDEPENDENT is a proof obligation (every permutation of the walk must agree), DEPENDENT needs two differing walks, and
UNDECIDED may only be rare: all three are held against a brute force over every permutation of small random cases.
"""
import functools
import itertools
import random

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import Slimm
from slimm_amd.synth import CONFIGS, make_workload
from tests.cases import holes_case, tiny_case
from tests.helpers import assert_profiles_match, partials_from_oracle
from tests.propagation_cases import (FOUR_CONTIG_AB, all_walks, canonical, default_walk, direct_hits, four_contig_case,
                                     partials, random_case, step2)

IND, DEP, UND = capi.PROPAGATION_INDEPENDENT, capi.PROPAGATION_DEPENDENT, capi.PROPAGATION_UNDECIDED


def _host_only(w, o):
    s = Slimm.for_workload(w, device=-1)
    assert s.set_coverage_columns(o.reads_count, o.uniq_reads_count, o.nz_cov, o.nz_uniq_cov, o.scalars["hits"],
                                  o.scalars["matches"])
    s.filter_alignments()
    s.set_partials(*partials_from_oracle(o, w.lineage(), s.dense_taxid))
    return s


def _stage1(s):
    return sorted(s.taxon_counts(1).items()), sorted(s.children_pairs(1))


def _equals_oracle(s, o):
    if s.taxon_counts(1) != o.taxon_count or s.children_pairs(1) != o.taxon_children:
        return False
    assert_profiles_match(s.write_abundance(), o.profile_tsv)   # equal counts and children: the profile follows
    return True


# ------------------------------------------------------------------------------------------------ the four-contig family
@pytest.mark.parametrize("rank", ["species", "family"])
@pytest.mark.parametrize("ab", FOUR_CONTIG_AB)
def test_four_contigs_are_dependent_and_one_walk_is_the_oracles(ab, rank):
    w = four_contig_case(*ab, rank=rank)
    o = run_workload(w, collect_bins=False)
    s = _host_only(w, o)
    with pytest.raises(capi.SlimmError):
        s.propagation_order()                       # before any propagation: an error, like the other result getters
    equal = {}
    for walk in (capi.WALK_DEFAULT, capi.WALK_REVERSED):
        s.set_propagation_walk(walk)
        s.get_reads_lca_count()
        assert s.propagation_order() == (DEP, [0])  # the verdict is about every walk, whichever was taken
        assert s.taxon_counts(0) == o.lca_direct and s.children_pairs(0) == o.lca_direct_children
        equal[walk] = _equals_oracle(s, o)
    assert sorted(equal.values()) == [False, True], equal
    print(f"four contigs {ab} {rank}: the oracle's walk is", "reversed" if equal[capi.WALK_REVERSED] else "default")


def test_four_contigs_recorded_counts():
    """The figures the round-6 review recorded for a = b = 1 at species rank."""
    w = four_contig_case(1, 1)
    o = run_workload(w, collect_bins=False)
    assert {t: o.taxon_count[t] for t in (10, 12, 13)} == {10: 12, 12: 5, 13: 5}
    s = _host_only(w, o)
    s.get_reads_lca_count()
    assert {t: s.taxon_counts(1)[t] for t in (10, 12, 13)} == {10: 11, 12: 6, 13: 5}
    s.set_propagation_walk(capi.WALK_DEFAULT, first=[10])   # species 10 before taxid 0: the oracle's walk
    s.get_reads_lca_count()
    assert _equals_oracle(s, o)


def test_walk_settings_survive_reset_and_the_verdict_does_not():
    w = four_contig_case(2, 3)
    o = run_workload(w, collect_bins=False)
    s = _host_only(w, o)
    s.set_propagation_walk(capi.WALK_REVERSED)
    s.get_reads_lca_count()
    reversed_result = _stage1(s)
    s.reset()
    with pytest.raises(capi.SlimmError):
        s.propagation_order()
    s.set_coverage_columns(o.reads_count, o.uniq_reads_count, o.nz_cov, o.nz_uniq_cov, o.scalars["hits"], o.scalars["matches"])
    s.filter_alignments()
    s.set_partials(*partials_from_oracle(o, w.lineage(), s.dense_taxid))
    s.get_reads_lca_count()
    assert _stage1(s) == reversed_result and s.propagation_order() == (DEP, [0])
    s.set_propagation_walk(capi.WALK_DEFAULT, first=[999, 31, 0, 0])   # unknown, uncounted, counted, repeated
    s.get_reads_lca_count()
    default_result = _stage1(s)
    assert default_result != reversed_result
    s.set_propagation_walk(capi.WALK_DEFAULT)                           # an empty list clears the priority
    s.get_reads_lca_count()
    assert _stage1(s) == default_result
    with pytest.raises(capi.SlimmError):
        s.set_propagation_walk(7)


# ------------------------------------------------------------------------------------------------ brute force
N_CASES = 1800


@functools.lru_cache(maxsize=None)
def _brute_force():
    """(workload, lineage, rank_of, lca, kids, has_hole, verdict, taxa, the results of every walk) per case, computed once."""
    rng = random.Random(20251017)
    out = []
    while len(out) < N_CASES:
        w, lineage, rank_of, reads, has_hole = random_case(rng)
        lca, kids = direct_hits(lineage, reads)
        if len(lca) > 6:
            continue
        s = Slimm.for_workload(w, device=-1)
        one = np.ones(w.n_refs, dtype=np.uint32)
        assert s.set_coverage_columns(one, one, one, one, w.n_refs, w.n_refs)
        s.filter_alignments()
        s.set_partials(*partials(lineage, s.dense_taxid, lca, kids))
        s.get_reads_lca_count()
        verdict, taxa = s.propagation_order()
        out.append((s, lineage, rank_of, lca, kids, has_hole, verdict, taxa, all_walks(lineage, rank_of, lca, kids)))
    return out


def test_verdicts_against_every_permutation():
    cases = _brute_force()
    holes = undecided = missed = 0
    tally = {IND: 0, DEP: 0, UND: 0}
    for s, lineage, rank_of, lca, kids, has_hole, verdict, taxa, walks in cases:
        differ = len(set(map(repr, walks.values()))) > 1
        tally[verdict] += 1
        holes += has_hole
        if verdict == IND:
            assert not differ, f"INDEPENDENT, but two walks differ: {lineage.tolist()} {lca} {kids}"
            assert taxa == []
        elif verdict == DEP:
            assert differ, f"DEPENDENT, but every walk agrees: {lineage.tolist()} {lca} {kids}"
        else:
            assert has_hole, f"UNDECIDED on a hole-free database: {lineage.tolist()} {lca} {kids}"
            undecided += 1
            missed += differ
        if verdict != IND:
            assert taxa and taxa == sorted(set(taxa)) and set(taxa) <= set(lca), (taxa, lca)
        if not has_hole:
            assert not differ                      # (the model's own claim: a consistent tree has one answer)
    print(f"{len(cases)} cases, {holes} with a hole: independent {tally[IND]}, dependent {tally[DEP]}, undecided {undecided} "
          f"({100.0 * undecided / max(holes, 1):.2f} % of the cases with a hole; {missed} of them do differ)")
    assert len(cases) >= 1500 and holes >= 500 and tally[DEP] >= 50
    assert undecided <= 0.06 * holes


def test_every_permutation_through_the_priority_list():
    """The library's own walk, position by position: first = a whole permutation leaves nothing to the chosen walk."""
    driven = 0
    for s, lineage, rank_of, lca, kids, has_hole, verdict, taxa, walks in _brute_force():
        if not 2 <= len(lca) <= 5 or (driven >= 40 and verdict == IND):
            continue
        for perm, want in walks.items():
            s.set_propagation_walk(capi.WALK_REVERSED, first=perm)
            s.get_reads_lca_count()
            assert _stage1(s) == (want[0], want[1]), (perm, lineage.tolist(), lca)
            assert s.propagation_order() == (verdict, taxa)
        # and the two walks without a list
        dw = default_walk(rank_of, lca)
        for walk, order in ((capi.WALK_DEFAULT, dw), (capi.WALK_REVERSED, dw[::-1])):
            s.set_propagation_walk(walk)
            s.get_reads_lca_count()
            assert _stage1(s) == canonical(*step2(lineage, rank_of, lca, kids, order))
        driven += 1
        if driven >= 90:
            break
    assert driven >= 50


# ------------------------------------------------------------------------------------------------ existing shapes
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_hole_free_config1_is_independent(seed):
    w = make_workload(CONFIGS["config1"], seed=seed)
    s = _host_only(w, run_workload(w, use_qnames=False, collect_bins=False))
    s.get_reads_lca_count()
    assert s.propagation_order() == (IND, [])


def _model_inputs(w, o):
    rank_of = {int(t): int(k) for t, k in zip(w.taxonomy.tax_id, w.taxonomy.tax_rank)}
    kids = {}
    for t, r in o.lca_direct_children:
        kids.setdefault(t, set()).add(r)
    return w.lineage(), rank_of, dict(o.lca_direct), kids


@pytest.mark.parametrize("mk", [tiny_case, holes_case])
def test_micro_cases_say_what_the_brute_force_says(mk):
    w = mk()
    o = run_workload(w, collect_bins=False)
    s = _host_only(w, o)
    s.get_reads_lca_count()
    verdict, taxa = s.propagation_order()
    walks = all_walks(*_model_inputs(w, o))
    differ = len(set(map(repr, walks.values()))) > 1
    print(f"{w.name}: verdict {verdict}, taxa {taxa}, {len(walks)} walks, differ: {differ}")
    assert not differ and (verdict, taxa) == (IND, [])


@pytest.mark.parametrize("seed", [4, 7])
def test_config1_with_holes_is_dependent_where_two_walks_differ(seed):
    w = make_workload(CONFIGS["config1"], seed=seed, hole_every=3)
    o = run_workload(w, use_qnames=False, collect_bins=False)
    s = _host_only(w, o)
    res = {}
    for walk in (capi.WALK_DEFAULT, capi.WALK_REVERSED):
        s.set_propagation_walk(walk)
        s.get_reads_lca_count()
        res[walk] = _stage1(s)
    verdict, taxa = s.propagation_order()
    differ = res[capi.WALK_DEFAULT] != res[capi.WALK_REVERSED]
    print(f"config1 hole_every=3 seed {seed}: verdict {verdict}, taxa {taxa}, default and reversed differ: {differ}")
    if differ:
        assert verdict == DEP
    assert (verdict == IND) == (taxa == [])


# ------------------------------------------------------------------------------------------------ the merged path
def test_merged_partials_give_the_same_verdict():
    """Two ranks' partial results of the four-contig case, summed the way the multi-rank path sums them (counts added,
    marks ORed, pairs united) and installed with set_partials: the verdict of one context on all records."""
    w = four_contig_case(3, 2)
    o = run_workload(w, collect_bins=False)
    whole = _host_only(w, o)
    whole.get_reads_lca_count()
    u2, lca, marks, pairs = partials_from_oracle(o, w.lineage(), whole.dense_taxid)
    lo = (u2 // 2, lca // 2, marks & 0x3, pairs[: len(pairs) // 2])
    hi = (u2 - lo[0], lca - lo[1], marks & ~np.uint32(0x3), pairs[len(pairs) // 2:])
    merged = Slimm.for_workload(w, device=-1)
    merged.set_coverage_columns(o.reads_count, o.uniq_reads_count, o.nz_cov, o.nz_uniq_cov, o.scalars["hits"], o.scalars["matches"])
    merged.filter_alignments()
    merged.set_partials(lo[0] + hi[0], lo[1] + hi[1], lo[2] | hi[2], np.union1d(lo[3], hi[3]))
    merged.get_reads_lca_count()
    assert merged.propagation_order() == whole.propagation_order() == (DEP, [0])
    assert _stage1(merged) == _stage1(whole)
