"""The antipodal ray caster's truths (tests/sampler_truth.py) and the C oracle
against them, on the CPU.

First the float truth (numpy, the kernel's order of operations) against the
exact truth (fractions.Fraction): equal counts wherever the ray is not within
1e-9 of a decision, points within rounding; on the dyadic box bit for bit.
Then oracle_antipodal_contacts against the float truth, bit for bit, at the
inputs where the rule can go wrong: hits spread over several tiles of 256 out
of depth order, three eps values, rays without a hit, a degenerate and a
parallel triangle, and the choice uniform at every edge of every slot.
tests/test_sampler_edges_gpu.py holds the kernel to the same truth."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sampler_truth as S  # noqa: E402

EPS = (0.0, 1e-5, 0.5)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def oracle_equals_truth(tri, o, d, u, eps):
    from oracle import oracle as O
    sec, cnt = O.antipodal_contacts(tri, o, d, u, eps)
    want_sec, want_cnt = S.ray_contacts(tri, o, d, u, eps)
    return np.array_equal(cnt, want_cnt) and np.array_equal(bits(sec), bits(want_sec))


@pytest.fixture(scope="module")
def shells():
    return {False: S.nested_shells(), True: S.nested_shells(shuffled=True)}


@pytest.fixture(scope="module")
def rays():
    return S.shell_rays(600)


def test_shells_and_rays_are_what_the_tests_need(shells, rays):
    """720 triangles; the rays meet 0, 2, 4 and 6 of them; in the shuffled order
    one ray's hits lie in different tiles of 256 and out of depth order"""
    o, d, u = rays
    assert shells[False].shape == (720, 9) and shells[True].shape == (720, 9)
    assert not np.array_equal(shells[False], shells[True])
    _, cnt = S.ray_contacts(shells[False], o, d, u, 0.0)
    assert set(np.unique(cnt)) == {0, 2, 4, 6}
    found = False
    for i in np.nonzero(cnt == 6)[0][:20]:
        for sign in (1.0, -1.0):
            hit, t = S.T.ray_tri(o[i], sign * d[i], shells[True])
            j = np.nonzero(hit)[0]
            if len(j) >= 2 and len(set(j // 256)) >= 2 and np.any(np.diff(t[j]) < 0):
                found = True
    assert found


@pytest.mark.parametrize("shuffled", [False, True])
def test_float_truth_against_exact_truth(shells, rays, shuffled):
    """300 rays on the shells: equal counts for every ray not within 1e-9 of a
    decision (a triangle's edge or vertex, t = 0, distance = eps, u * total an
    integer), at most 2 % of the rays left out by that rule.

    Measured: no ray of the 300 left out in either order, the nearest approach
    to a decision 1.9e-4; the largest point error 5.6e-16 (a few ulps of a
    coordinate near 1: t is rounded, then o + t d).  The bound is 16 times
    that, 8.9e-15, and has to stay below 1e-13."""
    o, d, u = (a[:300] for a in rays)
    measured = 5.6e-16
    for eps in (1e-5, 0.5):
        sec, cnt = S.ray_contacts(shells[shuffled], o, d, u, eps)
        xsec, xcnt, margin = S.ray_contacts_exact(shells[shuffled], o, d, u, eps)
        keep = margin >= 1e-9
        err = np.abs(sec - xsec)[keep].max()
        print(f"shuffled={shuffled} eps={eps}: left out {np.count_nonzero(~keep)} of {len(keep)}, nearest approach "
              f"{margin.min():.3g}, point error {err:.3g}")
        assert np.count_nonzero(~keep) <= 0.02 * len(keep)
        assert np.array_equal(cnt[keep], xcnt[keep])
        assert 16 * measured < 1e-13
        assert err <= 16 * measured


@pytest.mark.parametrize("eps", [0.0, 0.25, 0.5, 1.0])
def test_float_truth_equals_exact_truth_on_dyadic_box(eps):
    """every intermediate is exact: bit for bit, no ray left out -- rays through
    face centres (two triangles hit, at u + w == 1 and w == 0), edge midpoints,
    corners, along a face, from a point on a face (t == 0), and hits at exactly
    eps"""
    tri, o, d, u = S.dyadic_box()
    sec, cnt = S.ray_contacts(tri, o, d, u, eps)
    xsec, xcnt, margin = S.ray_contacts_exact(tri, o, d, u, eps)
    assert np.array_equal(cnt, xcnt)
    assert np.array_equal(bits(sec), bits(xsec))
    assert np.count_nonzero(margin == 0.0) >= 10            # the rays do sit on decisions
    if eps == 0.0:
        assert cnt[0] == 4 and cnt.max() >= 6 and cnt.min() == 0


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shuffled", [False, True])
def test_oracle_equals_truth_on_shells(shells, rays, shuffled, eps):
    o, d, u = rays
    assert oracle_equals_truth(shells[shuffled], o, d, u, eps)
    if eps == 0.5:                                           # the near shell's hits are gone
        _, c0 = S.ray_contacts(shells[shuffled], o, d, u, 0.0)
        _, c5 = S.ray_contacts(shells[shuffled], o, d, u, eps)
        assert np.all(c5 <= c0) and np.any(c5 < c0)


@pytest.mark.parametrize("eps", [0.0, 1e-5, 0.25, 0.5, 1.0])
def test_oracle_equals_truth_on_dyadic_box(eps):
    tri, o, d, u = S.dyadic_box()
    assert oracle_equals_truth(tri, o, d, u, eps)


def test_oracle_rays_without_a_hit(shells):
    from oracle import oracle as O
    o = np.array([[3.0, 0.0, 0.0], [0.0, 2.0, 2.0], [5.0, 5.0, 5.0]])
    d = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    u = np.array([0.0, 0.5, 1.0])
    for tri in (shells[True], shells[True][:0]):
        sec, cnt = O.antipodal_contacts(tri, o, d, u, 1e-5)
        assert np.array_equal(cnt, np.zeros(3, np.int32)) and np.array_equal(bits(sec), np.zeros((3, 3), np.int64))
        assert oracle_equals_truth(tri, o, d, u, 1e-5)


def test_oracle_degenerate_and_parallel_triangles(shells, rays):
    """a zero-area triangle (on the first ray, at the place of its first hit)
    and a triangle parallel to the first ray's direction change no answer"""
    o, d, u = (a[:64] for a in rays)
    sec0, cnt0 = S.ray_contacts(shells[False], o, d, u, 1e-5)
    at = o[0] + 0.5 * d[0]
    side = np.cross(d[0], [0.0, 0.0, 1.0])
    off = at + 0.1 * np.cross(d[0], side)
    flat = np.concatenate([at, at + d[0], at + 2.0 * d[0]])                 # collinear along the ray
    para = np.concatenate([off, off + d[0], off + side])                    # in a plane parallel to the ray
    point = np.concatenate([at, at, at])
    tri = np.concatenate([shells[False], flat[None], para[None], point[None]])
    sec, cnt = S.ray_contacts(tri, o, d, u, 1e-5)
    assert cnt[0] == cnt0[0] and np.array_equal(bits(sec[0]), bits(sec0[0]))
    assert oracle_equals_truth(tri, o, d, u, 1e-5)


@pytest.mark.parametrize("shuffled", [False, True])
def test_oracle_choice_rule_at_every_slot_edge(shells, rays, shuffled):
    """u at j / total, just below it, mid-slot, 0, just below 1 and exactly 1
    for every slot of every ray: the pick falls in the +d list, in the -d list,
    in the first tile and in the last"""
    o, d, u = rays
    _, cnt = S.ray_contacts(shells[shuffled], o, d, u, 1e-5)
    idx, us = S.u_sweep(cnt)
    assert len(idx) == 2 * cnt.sum() and us.min() == 0.0 and us.max() == 1.0
    assert oracle_equals_truth(shells[shuffled], o[idx], d[idx], us, 1e-5)
    sec, _ = S.ray_contacts(shells[shuffled], o[idx], d[idx], us, 1e-5)
    # the picks of one ray differ: every slot is reached
    six = np.nonzero(cnt == 6)[0][0]
    assert len(np.unique(bits(sec[idx == six]), axis=0)) == 6


def test_engine_refuses_unequal_lengths():
    """origin, direction and u_choice of different lengths are refused before
    any library is loaded (the kernel would read past the shorter ones)"""
    from mgs.core import engine
    tri = S.nested_shells()[:4]
    o, d, u = S.shell_rays(8)
    for bad in ((o, d[:7], u), (o, d, u[:7]), (o[:7], d, u), (o, d, u[:0])):
        with pytest.raises(ValueError, match="antipodal_contacts"):
            engine.antipodal_contacts(tri, *bad, 1e-5)
