"""mgs_antipodal_kernel on the MI355X (through mgs.core.engine) against the
numpy truth of tests/sampler_truth.py and the C oracle, bit for bit, at the
kernel's seams: ray counts around the block of 256 lanes, triangle counts
around the LDS tile of 256 (none, one, a full tile, a tile and one, three
tiles), hits of one ray in different tiles out of depth order, the dyadic box
whose rays sit on every decision, three eps values, and the choice uniform at
every edge of every slot."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sampler_truth as S  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def kernel_equals_truth_and_oracle(tri, o, d, u, eps):
    from mgs.core.engine import antipodal_contacts
    from oracle import oracle as O
    sec, cnt, ms = antipodal_contacts(tri, o, d, u, eps)
    tsec, tcnt = S.ray_contacts(tri, o, d, u, eps)
    osec, ocnt = O.antipodal_contacts(tri, o, d, u, eps)
    assert sec.shape == (len(o), 3) and cnt.dtype == np.int32 and ms > 0
    assert np.array_equal(cnt, tcnt) and np.array_equal(bits(sec), bits(tsec))
    assert np.array_equal(cnt, ocnt) and np.array_equal(bits(sec), bits(osec))
    return sec, cnt


@pytest.fixture(scope="module")
def shuffled():
    return S.nested_shells(shuffled=True)


@pytest.fixture(scope="module")
def rays():
    return S.shell_rays(600)


@pytest.mark.parametrize("ntri", [1, 255, 256, 257, 720])
def test_triangle_counts_around_the_tile(shuffled, rays, ntri):
    o, d, u = (a[:257] for a in rays)
    _, cnt = kernel_equals_truth_and_oracle(shuffled[:ntri], o, d, u, 1e-5)
    if ntri >= 255:
        assert cnt.max() >= 2


@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_ray_counts_around_the_block(shuffled, rays, n):
    o, d, u = (a[:n] for a in rays)
    kernel_equals_truth_and_oracle(shuffled, o, d, u, 1e-5)


def test_no_triangles(shuffled, rays):
    """ntri = 0: every count 0, every point zeros, as the oracle answers"""
    o, d, u = (a[:3] for a in rays)
    sec, cnt = kernel_equals_truth_and_oracle(shuffled[:0], o, d, u, 1e-5)
    assert np.array_equal(cnt, np.zeros(3, np.int32)) and np.array_equal(bits(sec), np.zeros((3, 3), np.int64))


@pytest.mark.parametrize("eps", [0.0, 1e-5, 0.25, 0.5, 1.0])
def test_dyadic_box(eps):
    tri, o, d, u = S.dyadic_box()
    kernel_equals_truth_and_oracle(tri, o, d, u, eps)


@pytest.mark.parametrize("eps", [0.0, 1e-5, 0.5])
@pytest.mark.parametrize("order", ["plain", "shuffled"])
def test_eps_values(rays, order, eps):
    kernel_equals_truth_and_oracle(S.nested_shells(shuffled=order == "shuffled"), *rays, eps)


def test_choice_rule_at_every_slot_edge(shuffled, rays):
    """the pick falls in the +d list, in the -d list, in the first tile and in
    the last; u * total lands on, just below and between the integers"""
    o, d, u = rays
    _, cnt = S.ray_contacts(shuffled, o, d, u, 1e-5)
    idx, us = S.u_sweep(cnt)
    sec, got = kernel_equals_truth_and_oracle(shuffled, o[idx], d[idx], us, 1e-5)
    assert np.array_equal(got, cnt[idx])
    six = np.nonzero(cnt == 6)[0][0]
    assert len(np.unique(bits(sec[idx == six]), axis=0)) == 6
