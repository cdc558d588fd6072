"""The contact sampler's truths (tests/sampler_truth.py) and the C oracle
against them, on the CPU: the seed neighbourhoods (splitmix64 keys, the order of
the picks, the nearest seed) over a grid of sizes, radii, keys and tip counts on
a lattice with duplicates and distances equal to the radius; the AdamW fit
against a torch float64 transcription of the reference's formulas whose
gradient is autograd's.  tests/test_contact_edges_gpu.py holds the kernels to
the same truths."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sampler_truth as S  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# -- seeds --------------------------------------------------------------------
def test_splitmix64_known_answers():
    """the published first outputs of SplitMix64 seeded with 0, and the array
    form against the integer form with the top bit set and at the wrap"""
    assert S.splitmix64_int(0) == 0xE220A8397B1DCDAF
    assert S.splitmix64_int(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    x = np.array([0, 1, 2**63, 2**63 + 12345, 2**64 - 1, 0x61C8864680B583EB], np.uint64)
    assert [int(v) for v in S._splitmix64(x)] == [S.splitmix64_int(int(v)) for v in x]
    for key in S.SEED_KEY:
        K = S.key_uniforms(key, 7)
        assert all(K[i, j] == S.key_uniform_int(key, i * 7 + j) for i in range(7) for j in range(7))
        assert K.min() >= 0.0 and K.max() < 1.0 and len(np.unique(K)) == 49


def test_seed_lattice_has_the_edges():
    s = S.seed_lattice(257)
    d = np.linalg.norm(s[:, None] - s[None], axis=-1)
    assert np.array_equal(s[0], s[1]) and np.count_nonzero(d == 0.0) > 257 and np.count_nonzero(d == 0.125) > 0


@pytest.mark.parametrize("k", S.SEED_K)
def test_oracle_seeds_equal_truth(k):
    """nn and sel over radius x key x ntip: k < ntip fills with the seed itself,
    k = 257 and 513 leave one seed in the last tile of 256, radius 0 admits
    nothing, 1e-9 only duplicates, 0.125 is a lattice distance (d < radius is
    strict), the keys 2^63 + 12345 and 2^64 - 1 have the top bit set"""
    from oracle import oracle as O
    s = S.seed_lattice(k)
    for radius in S.SEED_RADIUS:
        for key in S.SEED_KEY:
            for ntip in S.SEED_NTIP:
                nn, sel = O.contact_seeds(s, radius, key, ntip)
                tnn, tsel = S.seeds(s, radius, key, ntip)
                assert np.array_equal(nn, tnn), (radius, key, ntip)
                assert np.array_equal(sel, tsel), (radius, key, ntip)
    if k >= 255:            # the keys matter: another key, another pick
        assert not np.array_equal(S.seeds(s, 10.0, 0, 5)[1], S.seeds(s, 10.0, 99, 5)[1])
        assert not np.array_equal(S.seeds(s, 0.125, 0, 5)[1], S.seeds(s, 0.1250001, 0, 5)[1])


# -- the fit ------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    return S.fit_reference()


def test_truth_constants_are_the_products():
    from mgs.sampler import contact as C
    from mgs.sampler.kin.model import ShadowKinematicsModel
    d = C.kin_desc(ShadowKinematicsModel(), [0, 0, 0, 0, 0])
    assert (d.lr, d.b1, d.b2, d.eps, d.eps_root, d.weight_decay, d.w_cos) == \
        (S.LR, S.B1, S.B2, S.ADAM_EPS, 0.0, S.WEIGHT_DECAY, S.COS_WEIGHT)


def test_oracle_fit_against_torch_truth(reference):
    """oracle_contact_optimize against the autograd truth: six candidates, both
    contact-point orders, after 1, 5 and 20 steps; pos, joints, rot and loss
    within 64 times the truth's own sensitivity to a one-ulp change of its
    inputs (the two sides sum in different orders).

    Measured: sensitivity 4.4e-16 after 1, 5 and 20 steps (two ulps of a
    rotation entry near 1), so the bound is 2.8e-14, below 1e-12; the oracle is
    within 7.8e-16 of the truth (joints, 20 steps); the smallest assignment gap
    over the steps is 6.7e-5 with the first order and 2.2e-5 with the second,
    so none of the six candidates is left out; joints end on a range bound."""
    from mgs.sampler import contact as C
    from oracle import oracle as O
    S.check_fit(O.contact_optimize, C.kin_desc, reference)


def test_oracle_fit_zero_steps(reference):
    from mgs.sampler import contact as C
    from oracle import oracle as O
    S.check_fit_zero_steps(O.contact_optimize, C.kin_desc, reference)
