"""The planted instances of tests/fit_cases.py have the properties they are there for -- checked with the oracle alone, no
GPU: cluster sizes, cluster counts, the launch class of the segment, and whether a grid variant of the clustering would
accept the instance (the two conditions of grid_geometry in fit_stage.hip, restated here)."""
import math

import numpy as np
import pytest

from oracle import penet_oracle as O
from tests import fit_cases as F


def _all_cases():
    cases = F.edge_size_cases() + F.long_cases() + [F.many_cluster_case(), F.singleton_case()]
    cases += F.asym_far_cases() + F.asym_near_cases()
    cases += [F.fallback_case(n) for n in F.FALLBACK_SIZES]
    cases += F.ring_tie_cases()
    return cases


CASES = _all_cases()


def _grid_eligible(pts, R0, Rd):
    """grid_geometry: cell side g = R_max / 2 (+ margins), R_max from the farthest point; eligible if two points of one
    cell are always linked (g sqrt 2 <= 0.999 R0) and the bounding box needs at most 12 288 cells."""
    x, y = pts[:, 0], pts[:, 1]
    Rmax = (R0 + Rd * math.sqrt(float((x * x + y * y).max()))) * (1.0 + 1e-9) + 1e-12
    g = 0.5 * Rmax * (1.0 + 1e-6) + 1e-12
    cells = (math.floor((x.max() - x.min()) / g) + 1.0) * (math.floor((y.max() - y.min()) / g) + 1.0)
    return g * math.sqrt(2.0) <= 0.999 * R0 and cells <= 12288


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_has_its_planted_properties(case):
    lab = O.range_cluster_labels(case.pts[:, 0], case.pts[:, 1], case.R0, case.Rd)
    cnt = np.bincount(lab, minlength=case.n)
    roots = np.nonzero(cnt)[0]
    assert cnt[roots].tolist() == list(case.sizes)
    assert case.n_clusters == len(roots)
    if case.roots is not None:
        assert np.array_equal(roots, case.roots)
    assert _grid_eligible(case.pts, case.R0, case.Rd) == case.grid_ok
    assert case.seg_class == (0 if case.n > 16384 else 1 if case.n > 8192 else 2)


def test_the_cases_cover_what_they_are_named_for():
    by = {c.name: c for c in CASES}
    assert [c.sizes for c in F.edge_size_cases()] == [[m] for m in (64, 65, 2048, 2049, 4096, 4097, 6144, 6145, 8192, 8193)]
    assert by["edge8193"].seg_class == 1 and by["edge8192"].seg_class == 2
    one, mixed = F.long_cases()
    assert one.sizes == [16385] and one.seg_class == 0
    assert sorted(mixed.sizes) == [1] * 12 + [300, 16384] and mixed.seg_class == 0 and 16384 < mixed.n < 17500
    many = by["many533"]
    assert 512 < many.n_clusters < 1024 and sorted(many.sizes)[-4:] == [2, 65, 300, 2049]
    rank = {m: k for k, m in enumerate(many.sizes) if m > 1}         # rank of the root among the instance's roots
    assert rank[65] < 512 and min(rank[2], rank[300], rank[2049]) >= 512
    single = F.singleton_case()
    assert single.n_clusters > 1024 and set(single.sizes) == {1}
    for fam, ok in ((F.asym_far_cases(), False), (F.asym_near_cases(), True)):
        assert {c.n_clusters for c in fam} == {1, 2} and all(c.grid_ok == ok for c in fam)
    assert [F.fallback_case(n).n for n in F.FALLBACK_SIZES] == [300, 4096, 4097, 61440, 61441]
    assert not any(F.fallback_case(n).grid_ok for n in F.FALLBACK_SIZES)


@pytest.mark.parametrize("dtheta_deg,n_theta", F.TIE_HEADINGS)
def test_ring_ties_put_more_than_one_heading_in_the_band(dtheta_deg, n_theta):
    """Every (case, heading count) of the tie test has at least two headings within the band of the two-tier search, so
    the GPU test cannot pass without tier 2; each case is ONE cluster under the default R0, Rd.  Above 64 headings the
    in-band set reaches into the second heading slot of a lane of k_fit_tiny."""
    assert O.Params().dtheta_deg == 1.0 and (F.FitCase.R0, F.FitCase.Rd) == (O.Params().R0, O.Params().Rd)
    assert len(np.arange(0.0, np.pi / 2.0 - np.deg2rad(dtheta_deg), np.deg2rad(dtheta_deg))) == n_theta
    cases = F.ring_tie_cases()
    assert [c.sizes for c in cases] == [[n] for n in (64, 65, 2048, 2049, 4097)]
    for c in cases:
        assert (c.R0, c.Rd) == (F.FitCase.R0, F.FitCase.Rd)
        lab = O.range_cluster_labels(c.pts[:, 0], c.pts[:, 1], c.R0, c.Rd)
        assert not lab.any(), c.name                                 # one cluster, root 0
        band = F.tier1_band(c.pts, dtheta_deg)
        assert len(band) >= 2, (c.name, n_theta, band)
        if n_theta > 64:
            assert band.max() >= 64, (c.name, n_theta, band)
        if (n_theta, c.name) in F.TIE_DISAGREE:                      # both indices are members of the tied set
            assert set(F.TIE_DISAGREE[n_theta, c.name]) <= set(band.tolist()), (c.name, n_theta, band)


def test_the_ring_ties_left_out_leave_every_size_and_heading_count_covered():
    kept = {n: [c.name for c in F.ring_tie_cases_at(n)] for _, n in F.TIE_HEADINGS}
    assert sum(len(v) for v in kept.values()) == 20 - len(F.TIE_DISAGREE) == 14
    assert all(len(v) >= 2 for v in kept.values())
    assert set().union(*kept.values()) == {"tie%d" % n for n in F.TIE_SIZES}
    assert "tie64" in kept[128]                                      # the second heading slot of k_fit_tiny's lanes
