"""The contact sampler's kernels on the MI355X (through mgs.core.engine) at
their seams: mgs_fps_kernel around its 1024 lanes and with every pick tied,
mgs_seeds_kernel against the numpy truth over sizes around its tile of 256,
tip counts above the seed count, radii equal to a distance and 64-bit keys with
the top bit set, mgs_contact_opt_kernel against the C oracle bit for bit
around its block of 64 lanes at 0, 1 and 150 steps, and against the autograd
truth of tests/sampler_truth.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_truth as C  # noqa: E402
import sampler_truth as S  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# -- farthest-point pick ------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_fps_around_the_lane_count(n):
    from mgs.core.engine import contact_fps
    x = np.random.default_rng(n).normal(size=(n, 3)) * 0.05
    x[n - 1] = 10.0                       # the second pick is the last index
    idx, ms = contact_fps(x, 8)
    assert np.array_equal(idx, C.brute_fps(x, 8)) and idx[1] == n - 1 and ms > 0


def test_fps_every_pick_tied():
    """70 copies of one point: every pick after the first ties at distance 0,
    and the first maximum is index 0"""
    from mgs.core.engine import contact_fps
    x = np.tile([0.3, -0.2, 0.1], (70, 1))
    idx, _ = contact_fps(x, 5)
    assert np.array_equal(idx, C.brute_fps(x, 5)) and np.array_equal(idx, np.zeros(5, np.int32))


# -- seeds --------------------------------------------------------------------
@pytest.mark.parametrize("k", S.SEED_K)
def test_seeds_equal_truth(k):
    """k = 4 < ntip = 5 gives the seed-itself slots, k = 257 and 513 a last
    tile of one seed, the key 2^64 - 1 goes through the ctypes boundary"""
    from mgs.core.engine import contact_seeds
    s = S.seed_lattice(k)
    for radius in S.SEED_RADIUS:
        for key in S.SEED_KEY:
            for ntip in S.SEED_NTIP:
                nn, sel, _ = contact_seeds(s, radius, key, ntip)
                tnn, tsel = S.seeds(s, radius, key, ntip)
                assert nn.dtype == np.int32 and sel.shape == (k, ntip)
                assert np.array_equal(nn, tnn), (radius, key, ntip)
                assert np.array_equal(sel, tsel), (radius, key, ntip)


# -- the fit ------------------------------------------------------------------
@pytest.fixture(scope="module")
def candidates():
    from mgs.sampler.kin.model import ShadowKinematicsModel
    kin = ShadowKinematicsModel()
    return kin, S.fit_case(kin, n=130, seed=9)


@pytest.mark.parametrize("iters", [0, 1, 150])
@pytest.mark.parametrize("order", S.FIT_ORDERS, ids=["21012", "01201"])
def test_fit_equals_oracle_bit_for_bit(candidates, order, iters):
    """n around the block of 64 lanes; the bits of the float64 outputs, so that
    no NaN passes for equal or for unequal"""
    from mgs.core.engine import contact_optimize
    from mgs.sampler import contact as K
    from oracle import oracle as O
    kin, case = candidates
    desc = K.kin_desc(kin, order, iters=iters)
    for n in (1, 63, 64, 65, 130):
        R, p, Tg, N = (a[:n] for a in case)
        g = contact_optimize(desc, R, p, Tg, N)
        o = O.contact_optimize(desc, R, p, Tg, N)
        for key in ("rot", "pos", "joints", "loss"):
            assert g[key].shape == o[key].shape and np.isfinite(g[key]).all(), (n, key)
            assert np.array_equal(bits(g[key]), bits(o[key])), (n, key)


@pytest.fixture(scope="module")
def reference():
    return S.fit_reference()


def test_fit_against_torch_truth(reference):
    """the kernel against the autograd truth, the bound and the conditions of
    tests/test_contact_truth.py::test_oracle_fit_against_torch_truth (64 times
    the truth's one-ulp sensitivity of 4.4e-16: 2.8e-14).  Measured: the kernel
    is within 7.8e-16 of the truth (joints, 20 steps), the oracle's own figures;
    smallest assignment gap 2.2e-5, no candidate left out."""
    from mgs.core.engine import contact_optimize
    from mgs.sampler import contact as K
    S.check_fit(contact_optimize, K.kin_desc, reference)


def test_fit_zero_steps(reference):
    from mgs.core.engine import contact_optimize
    from mgs.sampler import contact as K
    S.check_fit_zero_steps(contact_optimize, K.kin_desc, reference)
