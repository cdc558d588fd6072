"""Scene cloud, host side (no GPU): the numpy truth the GPU tests compare
against (tests/cloud_truth.py) checked against numpy's own floor_divide, the
host voxel function and a sweep; the wrappers' argument checks; the CLI key."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_truth as C  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("b", [0.002, 0.0123])
def test_cell_rule_is_numpys_floor_divide(b):
    rng = np.random.default_rng(11)
    a = C.boundary_values(b, rng, 200000)
    k = np.arange(0, 400, dtype=np.float64) * b
    a = np.concatenate([a, k, np.nextafter(k, np.inf), np.nextafter(k, -np.inf)[1:]])
    want = np.floor_divide(a, b)
    assert np.array_equal(C.cells(a, b), want.astype(np.int64))
    # the rule is needed: the plain quotient's floor is another function on these inputs
    assert np.any(np.floor(a / b) != want)


def same_voxels(got, want_p, want_f):
    return (got[0].shape == want_p.shape and np.array_equal(bits(got[0]), bits(want_p))
            and got[1].dtype == np.float32 and np.array_equal(got[1].view(np.int32), want_f.view(np.int32)))


@pytest.mark.parametrize("voxel_size", [0.002, 0.0123])
def test_truth_voxels_equal_the_host_function(voxel_size):
    from mgs.util.img_proc import voxel_downsample_pcd
    P, F, keep = C.adversarial_cloud()
    assert 4500 <= len(P) <= 5500 and P.dtype == np.float64 and F.dtype == np.float32
    assert len(np.unique(P, axis=0)) < len(P)                                       # duplicates
    for k in (None, keep):
        Pk, Fk = (P, F) if k is None else (P[k], F[k])
        wp, wf = voxel_downsample_pcd(Pk, Fk, voxel_size)
        got = C.voxels(P, F, voxel_size, k)
        assert same_voxels(got, wp, wf)
        assert got[2].sum() == len(Pk) and len(wp) < len(Pk)
        if voxel_size == 0.002 and k is None:
            assert got[2].max() == 300                                              # the crowded voxel
    # no features, one point, nothing kept
    got = C.voxels(P, np.zeros((len(P), 0), np.float32), voxel_size)
    assert np.array_equal(bits(got[0]), bits(voxel_downsample_pcd(P, np.zeros((len(P), 0), np.float32), voxel_size)[0]))
    assert np.array_equal(C.voxels(P[:1], F[:1], voxel_size)[0], P[:1])
    assert len(C.voxels(P, F, voxel_size, np.zeros(len(P), bool))[0]) == 0


def test_bucketed_pick_equals_the_sweep_on_a_surface():
    x = C.surface_cloud()
    n, k = 4000, 600
    assert x.shape == (n, 3)
    want = C.brute_fps(x, k)
    got, nevals, nbucket = C.bucket_fps(x, k, 0.016)
    assert np.array_equal(got, want) and len(set(want.tolist())) == k
    assert nbucket > 100
    assert 0 < nevals < n * (k - 1)
    assert nevals < 0.1 * n * (k - 1)              # what pruning is for (the prototype needed 1.5 %)


def test_bucketed_pick_equals_the_sweep_with_ties():
    x = C.lattice()
    n = len(x)
    assert n == 315 + 105
    want = C.brute_fps(x, n)
    for bucket in (0.016, 0.004, 1.0, 1e-5):
        got, _, nbucket = C.bucket_fps(x, n, bucket)
        assert np.array_equal(got, want), bucket
        assert nbucket == {0.016: 2, 0.004: 5 * 4 * 3, 1.0: 1, 1e-5: 315}[bucket]
    # every distinct point is taken before any duplicate's running minimum (0) can win
    assert len(np.unique(x[want[:315]], axis=0)) == 315


def test_bucket_side_doubles_until_the_grid_fits():
    x = C.surface_cloud(500)
    side, dims, flat = C.bucket_grid(x, 1e-6, max_cells=1 << 12)
    assert side == 1e-6 * 2 ** round(np.log2(side / 1e-6)) and dims.prod() <= 1 << 12 < (2 * dims).prod()
    assert flat.min() >= 0 and flat.max() < dims.prod()
    assert np.array_equal(C.bucket_fps(x, 50, 1e-6, max_cells=1 << 12)[0], C.brute_fps(x, 50))


def test_wrappers_reject_bad_arguments():
    """shape and dtype errors are ValueErrors raised before the library is loaded"""
    from mgs.core import engine
    P = np.zeros((5, 3))
    F = np.zeros((5, 3), np.float32)
    for args, kw in [((np.zeros((5, 2)), F), {}), ((np.zeros(15), None), {}), ((P, F[:4]), {}),
                     ((P, F.astype(np.float64)), {}), ((P, F), dict(keep=np.ones(4, bool))),
                     ((P, F), dict(keep=np.ones(5, np.float64))), ((P, F), dict(voxel_size=0.0)),
                     ((P, F), dict(voxel_size=np.inf)), ((P, F), dict(voxel_size=np.nan))]:
        with pytest.raises(ValueError):
            engine.scan_voxels(*args, **kw)
    for args in [(np.zeros((5, 2)), 2, 0.01), (P, 6, 0.01), (P, -1, 0.01), (P, 2, 0.0), (P, 2, -1.0), (P, 2, np.inf)]:
        with pytest.raises(ValueError):
            engine.scan_fps(*args)
    S = {}
    good = dict(scene_arrays=S, cam_pos=np.zeros((2, 3)), cam_rot=np.tile(np.eye(3), (2, 1, 1)), width=4, height=4, fx=5.0,
                fy=5.0, cx=2.0, cy=2.0, extrinsics=np.tile(np.eye(4), (2, 1, 1)), pfx=5.0, pfy=5.0, pcx=2.0, pcy=2.0,
                colors=np.zeros((3, 3)), num_points=8)
    for bad in (dict(extrinsics=np.eye(4)[None]), dict(cam_rot=np.eye(3)[None]), dict(colors=np.zeros((3, 4))),
                dict(colors=np.zeros(9)), dict(num_points=-1), dict(voxel_size=0.0), dict(region=np.zeros(5)),
                dict(width=-4)):
        with pytest.raises(ValueError):
            engine.scan_cloud(**dict(good, **bad))


def test_cli_cloud_key(monkeypatch, tmp_path):
    from mgs.cli import render_scene_processed as R
    from mgs.cli._hydra import compose
    assert R.cloud_path(compose("render_scene_proc", [])) == "host"
    assert R.cloud_path(compose("render_scene_proc", ["cloud=host"])) == "host"
    assert R.cloud_path(compose("render_scene_proc", ["cloud=device"])) == "device"
    # refused before the input directory is even looked at
    monkeypatch.setenv("MGS_INPUT_DIR", str(tmp_path / "missing"))
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path / "out"))
    with pytest.raises(ValueError, match="banana"):
        R.run(["gripper=robotiq_2f_85", "id=0", "cloud=banana"])
    assert not (tmp_path / "out").exists()


def test_header_declares_the_cloud_entries():
    from mgs.core import abi, engine
    txt = re.sub(r"/\*.*?\*/", "", open(abi.HEADER).read(), flags=re.S)
    for f in ("mgs_scan_voxels", "mgs_scan_fps", "mgs_scan_cloud"):
        assert re.search(r"^int %s\(" % f, txt, re.M), f
    assert abi.MGS["MGS_ABI_VERSION"] == 24
    assert abi.MGS["MGS_CLOUD_MAX_CELLS"] == 1 << 28 and abi.MGS["MGS_CLOUD_FPS_MAX_CELLS"] == C.FPS_MAX_CELLS
    assert len(engine.CLOUD_STATS) <= 8 and len(engine.CLOUD_STAGES) == 4
