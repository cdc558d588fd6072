"""Scene scan on the MI355X (csrc/mgs_scan.hip through the C-ABI) against the
numpy truth of tests/scan_truth.py: depth, segmentation, face ids and the
per-pixel triangle-test counts bit for bit, the point-cloud step bit for bit,
then ClutterTableEnv.scan and the render_scene_processed CLI end to end."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import scan_truth as T  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 37, 29      # no multiple of the 16 x 16 tile; three tiles across, two down


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def render(S, pos, R, width, height):
    from mgs.core.engine import scan_render
    f = T.focal(height)
    return scan_render(S, pos, R, width, height, f, f, width / 2, height / 2)


def check_parity(got, want):
    for k in ("seg", "tri", "ntest"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["depth"]), bits(want["depth"]))
    depth, seg, tri = want["brute"]
    assert np.array_equal(got["seg"], seg) and np.array_equal(got["tri"], tri)
    assert np.array_equal(bits(got["depth"]), bits(depth))


@pytest.fixture(scope="module")
def small():
    S = T.small_scene().arrays()
    pos, R = T.small_cameras()
    return S, pos, R, T.truth(S, pos, R, W, H)


@pytest.fixture(scope="module")
def small_gpu(small):
    S, pos, R, _ = small
    return render(S, pos, R, W, H)


def test_parity_small_scene(small, small_gpu):
    _, _, _, want = small
    seg = want["seg"]
    # what the scene is there for: every drawable kind seen, rays that miss
    # everything in the low views, and the camera inside the table box seeing the box's
    # inner faces wherever it looks (but for a mug that dips into the table)
    assert set(np.unique(seg[:3])) >= {-1, 10, 11, 12, 13, 14, 15}
    assert np.mean(seg[3] == 10) > 0.9 and np.all(want["depth"][3] > 0)
    assert (seg[0] == -1).any() and (seg[2] == -1).any()
    check_parity(small_gpu, want)
    assert small_gpu["kernel_ms"] > 0


def test_parity_deep_tree():
    """an icosahedron subdivided 4 times (5120 faces, a tree 11 levels deep)
    over the table, 2 views at 48 x 48; the tree prunes: over the pixels that
    hit the mesh the triangle tests stay below a sweep's 5120 per pixel"""
    from mgs.scan.scene import ScanScene
    v, f = T.icosphere(4, radius=0.08)
    assert len(f) == 5120
    sc = ScanScene()
    sc.add_box(0, [0.0, 0.0, -0.02], None, [10.0, 10.0, 0.02])
    sc.add_mesh(1, [0.01, -0.02, 0.1], T.rot([3, 1, 2], 0.9), v, f)
    S = sc.arrays()
    pos, R = T.fibonacci_cameras(4, which=(1, 2))
    want = T.truth(S, pos, R, 48, 48)
    hit = want["seg"] == 1
    assert hit.sum() > 100
    assert 0 < want["ntest"][hit].sum() < 5120 * hit.sum()          # the truth first, on the CPU
    got = render(S, pos, R, 48, 48)
    check_parity(got, want)
    assert 0 < got["ntest"][got["seg"] == 1].sum() < 5120 * (got["seg"] == 1).sum()


@pytest.mark.parametrize("iters", [0, 1, 5])
def test_scan_points(small, small_gpu, iters):
    from mgs.core.engine import scan_points
    _, pos, R, want = small
    E = np.tile(np.eye(4), (len(pos), 1, 1))
    E[:, :3, :3], E[:, :3, 3] = R, pos
    fx, fy, cx, cy = 73.0, T.focal(H), W / 2, H / 2            # fx != fy, as the reference's intrinsics
    P, keep = T.points(want["depth"], want["seg"], E, fx, fy, cx, cy, iters)
    gP, gkeep, ms = scan_points(small_gpu["depth"], small_gpu["seg"], E, fx, fy, cx, cy, erode_iters=iters)
    assert np.array_equal(bits(gP), bits(P)) and np.array_equal(gkeep, keep)
    assert keep.any() and not keep.all() and ms > 0
    if iters == 0:      # the mask alone: every hit pixel whose point is in the region
        assert keep.sum() > T.points(want["depth"], want["seg"], E, fx, fy, cx, cy, 5)[1].sum()
    # an explicit region replaces the reference's
    region = np.array([-0.1, -0.2, 0.001, 0.2, 0.1, 0.5])
    _, keep2 = T.points(want["depth"], want["seg"], E, fx, fy, cx, cy, iters, region)
    assert np.array_equal(scan_points(small_gpu["depth"], small_gpu["seg"], E, fx, fy, cx, cy, iters, region)[1], keep2)


def test_bad_arguments(small):
    from mgs.core import abi
    from mgs.core.engine import load_library
    from mgs.scan.scene import pack_scene
    L = load_library()
    S, pos, R, _ = small
    scene, keep = pack_scene(S)
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    n = 4 * 4
    depth, seg, tri = np.full(n, 7.0), np.full(n, 7, np.int32), np.full(n, 7, np.int32)
    cp, cr = np.ascontiguousarray(pos[:1]), np.ascontiguousarray(R[:1])

    def call(scene_ptr, nview, w, h):
        return L.mgs_scan_render(0, scene_ptr, nview, cp.ctypes.data_as(pd), cr.ctypes.data_as(pd), w, h, 5.0, 5.0,
                                 2.0, 2.0, depth.ctypes.data_as(pd), seg.ctypes.data_as(pi), tri.ctypes.data_as(pi),
                                 None, None)
    for args in ((None, 1, 4, 4), (ctypes.byref(scene), -1, 4, 4), (ctypes.byref(scene), 1, -4, 4),
                 (ctypes.byref(scene), 1, 4, -4)):
        assert call(*args) == abi.MGS["MGS_EINVAL"], args
        assert b"mgs_scan_render" in L.mgs_last_error()
    # a scene whose skip index points backwards is refused before anything runs
    bad = dict(S, node_skip=S["node_skip"].copy())
    bad["node_skip"][3] = 1
    bscene, bkeep = pack_scene(bad)
    assert call(ctypes.byref(bscene), 1, 4, 4) == abi.MGS["MGS_EINVAL"] and b"skip" in L.mgs_last_error()
    assert np.all(depth == 7.0) and np.all(seg == 7) and np.all(tri == 7)      # nothing was written
    pts, kp = np.zeros(3 * n), np.zeros(n, np.uint8)
    E = np.eye(4)

    def points(nview, w, h, iters):
        return L.mgs_scan_points(0, nview, w, h, depth.ctypes.data_as(pd), seg.ctypes.data_as(pi), E.ctypes.data_as(pd),
                                 5.0, 5.0, 2.0, 2.0, iters, None, pts.ctypes.data_as(pd),
                                 kp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None)
    for args in ((-1, 4, 4, 5), (1, -4, 4, 5), (1, 4, -4, 5), (1, 4, 4, -1)):
        assert points(*args) == abi.MGS["MGS_EINVAL"], args
    assert L.mgs_scan_points(0, 1, 4, 4, None, seg.ctypes.data_as(pi), E.ctypes.data_as(pd), 5.0, 5.0, 2.0, 2.0, 5,
                             None, pts.ctypes.data_as(pd), kp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                             None) == abi.MGS["MGS_EINVAL"]
    # and a valid call still works afterwards
    assert call(ctypes.byref(scene), 1, 4, 4) == 0 and not np.all(seg == 7)


# -- the env and the CLI --------------------------------------------------------
@pytest.fixture(scope="module")
def cenv():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_clutter_scene import make_env
    from mgs.env.clutter_table import ClutterTableEnv
    env = make_env()
    z = np.load(os.path.join(HERE, "golden", "clutter_scene.npz"))
    return ClutterTableEnv.from_dict({"gripper": env.gripper, "objects": env.objects,
                                      "env_state": {"state": z["state"]}})


def test_env_scan_end_to_end(cenv):
    from mgs.core.mjcf import load_mesh_bytes
    n, w, h = 3, 64, 64
    rgbd, extr, masks, seg = cenv.scan(num_images=n, width=w, height=h)
    assert rgbd.shape == (n, h, w, 4) and rgbd.dtype == np.float32
    assert extr.shape == (n, 4, 4) and extr.dtype == np.float64
    assert masks.shape == (n, h, w) and masks.dtype == bool
    assert seg.shape == (n, h, w) and seg.dtype == np.int32
    assert rgbd[..., :3].min() >= 0 and rgbd[..., :3].max() <= 1
    assert np.array_equal(masks, T.erode(seg != -1, 5)) and masks.any()
    assert np.all(rgbd[..., :3][seg == 0] == 0.5) and np.all(rgbd[seg == -1] == 0)
    assert set(np.unique(seg)) >= {0, 2, 3, 4, 5, 6}, "the pile's five objects and the table are in view"
    # the point of every masked pixel, along its own ray (pixel centre, f = fy on both axes)
    K = cenv.get_render_intrinsics()
    v, r, c = np.nonzero(masks)
    z = rgbd[v, r, c, 3].astype(np.float64)
    cam = np.stack([(c + 0.5 - K[0, 2]) * z / K[0, 0], (r + 0.5 - K[1, 2]) * z / K[1, 1], z, np.ones_like(z)], axis=1)
    P = np.sum(extr[v] * cam[:, None, :], axis=2)[:, :3]
    s = seg[v, r, c]
    assert (s == 0).sum() > 100 and np.abs(P[s == 0, 2]).max() <= 1e-5          # the table top is z = 0
    tri = cenv.last_scan["tri"][v, r, c]
    assert np.all((tri >= 0) == (s >= 2)) and not (s == 1).any()
    q = cenv.split_state(cenv.get_state())["qpos"]
    from mgs.scan.scene import quat_to_mat
    checked = 0
    for k, (o, (_, qs, _)) in enumerate(zip(cenv.objects, cenv._obj_slices())):
        sel = s == 2 + k
        if not sel.any():
            continue
        path = os.path.join(o.asset_dir, o.info()["original_file"])
        verts, faces = load_mesh_bytes(open(path, "rb").read(), path)
        world = verts @ quat_to_mat(q[qs][3:7] / np.linalg.norm(q[qs][3:7])).T + q[qs][:3]
        d = T.point_tri_dist(P[sel], world[faces[tri[sel]]])
        assert d.max() <= 1e-5, (o.name, d.max())
        checked += int(sel.sum())
    assert checked > 100
    # the reference's intrinsics go with the last scan's image size
    Kref = cenv.get_camera_intrinsics()
    assert Kref[1, 1] == K[1, 1] and Kref[0, 0] == pytest.approx(32 / np.tan(45 * np.pi / 720))


def test_render_scene_processed_cli(cenv, tmp_path, monkeypatch, capsys):
    from mgs.cli import render_scene_processed
    from mgs.env.selector import save_scene
    d = tmp_path / "in" / "Robotiq2f85Gripper" / "scene_000"
    d.mkdir(parents=True)
    save_scene(d / "scene.npz", cenv.to_dict())
    monkeypatch.setenv("MGS_INPUT_DIR", str(tmp_path / "in"))
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path / "out"))
    render_scene_processed.run(["gripper=robotiq_2f_85", "id=0", "num_images=4", "width=64", "height=64",
                                "num_points=256"])
    z = np.load(tmp_path / "out" / "Robotiq2f85Gripper" / "scene_000" / "scene_pcd.npz")
    P, C = z["points"], z["colors"]
    assert P.dtype == np.float32 and C.dtype == np.float32
    assert P.ndim == 2 and P.shape[1] == 3 and 0 < len(P) <= 256 and C.shape == (len(P), 3)
    lo, hi = np.float32([-0.25, -0.25, -0.01]), np.float32([0.25, 0.25, 1.0])
    assert np.all(P >= lo) and np.all(P <= hi)
    assert len(np.unique(P, axis=0)) == len(P)
    if len(P) < 256:
        assert "all kept" in capsys.readouterr().out
