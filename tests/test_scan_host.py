"""Scene scan, host side (no GPU): the threaded BVH (mgs/scan/bvh.py), the
numpy truth the GPU tests compare against (tests/scan_truth.py: traversal ==
brute force, bit for bit), the camera conventions, the erosion, the host
point-cloud processing and the two C-ABI declarations."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import scan_truth as T  # noqa: E402

MESHES = {
    "orange": lambda: T.shipped_mesh("YCB", "017_orange", "textured.obj"),
    "mug": lambda: T.shipped_mesh("GoogleScannedObjects", "Synthetic_Mug_Body", "model.obj"),
    "one": lambda: T.ONE_TRIANGLE,
    "seven": lambda: T.SEVEN_TRIANGLES,
}
NFACES = {"orange": 320, "mug": 92, "one": 1, "seven": 7}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_bvh_invariants(name):
    from mgs.scan.bvh import LEAF_MAX, build_bvh
    v, f = MESHES[name]()
    assert len(f) == NFACES[name]
    b = build_bvh(v, f)
    n = b.nnode
    assert n >= 1 and b.box.shape == (n, 6) and b.tri.shape == (len(f), 9)
    leaves = np.nonzero(b.count > 0)[0]
    # every face in exactly one leaf, leaves of at most LEAF_MAX = 4 faces
    assert LEAF_MAX == 4 and b.count.max() <= 4
    slots = np.concatenate([np.arange(b.first[i], b.first[i] + b.count[i]) for i in leaves])
    assert sorted(slots) == list(range(len(f)))
    assert sorted(b.face) == list(range(len(f)))
    assert np.array_equal(b.tri, np.asarray(v, np.float64)[np.asarray(f)[b.face]].reshape(-1, 9))
    # skip indices forward and within range; an inner node has its first child
    idx = np.arange(n)
    assert np.all(b.skip > idx) and np.all(b.skip <= n) and b.skip[0] == n
    assert np.all(idx[b.count == 0] + 1 < n)
    # each padded box contains the vertices of its subtree (nodes i .. skip[i] - 1)
    assert b.pad > 0
    for i in range(n):
        sub = [k for k in range(i, b.skip[i]) if b.count[k] > 0]
        pts = np.concatenate([b.tri[b.first[k]:b.first[k] + b.count[k]].reshape(-1, 3) for k in sub])
        assert np.all(pts.min(0) > b.box[i, :3]) and np.all(pts.max(0) < b.box[i, 3:]), i
        # and is no looser than the padding
        assert np.allclose(pts.min(0) - b.box[i, :3], b.pad, rtol=0, atol=1e-15 + 1e-3 * b.pad)


def test_instances_share_one_bvh():
    S = T.small_scene()
    assert len(S.meshes) == 3 and S.mesh == [-1, -1, 0, 1, 1, 2]
    a = S.arrays()
    assert a["mesh_tri0"].tolist() == [0, 320, 412, 413]


def test_traversal_equals_brute_force():
    """3 views at 24 x 24 of the small scene: (seg, tri, depth) of the threaded
    traversal == the sweep over every triangle, bit for bit"""
    S = T.small_scene().arrays()
    pos, R = T.fibonacci_cameras(3)
    r = T.truth(S, pos, R, 24, 24)
    depth, seg, tri = r["brute"]
    assert np.array_equal(r["seg"], seg) and np.array_equal(r["tri"], tri)
    assert np.array_equal(r["depth"].view(np.int64), depth.view(np.int64))
    # the views see every drawable kind and the sky, and the tree pruned
    assert set(np.unique(seg)) >= {-1, 10, 12, 13, 14}
    assert np.all((tri >= 0) == (seg >= 12))
    assert 0 < r["ntest"].sum() < 413 * seg.size


def test_box_from_inside_and_sphere_roots():
    """a camera inside a box sees the box's exit; a ray through a sphere takes
    the smallest positive root, from inside the far one"""
    from mgs.scan.scene import ScanScene
    sc = ScanScene()
    sc.add_box(0, [0, 0, 0], None, [1.0, 2.0, 3.0])
    S = sc.arrays()
    o, d = np.zeros((3, 3)), np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])   # zero components: inside tests
    depth, seg, tri = T.render_brute(S, o, d, (3,))
    assert depth.tolist() == [1.0, 3.0, 2.0] and seg.tolist() == [0, 0, 0] and tri.tolist() == [-1, -1, -1]
    o = np.array([[5.0, 0, 0], [5.0, 0, 0], [5.0, 2.5, 0]])
    d = np.array([[-1.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0]])       # entry, behind the ray, beside the box
    depth, seg, _ = T.render_brute(S, o, d, (3,))
    assert depth.tolist() == [4.0, 0.0, 0.0] and seg.tolist() == [0, -1, -1]
    sp = ScanScene()
    sp.add_sphere(7, [0, 0, 5.0], 1.0)
    o, d = np.array([[0.0, 0, 0], [0, 0, 5.0], [0, 0, 7.0]]), np.array([[0.0, 0, 1]] * 3)
    depth, seg, _ = T.render_brute(sp.arrays(), o, d, (3,))
    assert depth.tolist() == [4.0, 1.0, 0.0] and seg.tolist() == [7, 7, -1]


# -- camera -------------------------------------------------------------------
def test_fibonacci_positions():
    from mgs.util.camera import fibonacci_sphere
    # y = 1 - 2 i / 3, radius = sqrt(1 - y^2), theta = i pi (3 - sqrt 5): (cos theta r, y, sin theta r)
    want = [[0.0, 1.0, 0.0],
            [-0.6951980452, 1 / 3, 0.6368583569],
            [0.0824257637, -1 / 3, -0.9391990643],
            [0.0, -1.0, 0.0]]
    got = np.array([fibonacci_sphere(4, i) for i in range(4)])
    assert np.allclose(got, want, rtol=0, atol=1e-9)
    assert np.allclose(np.linalg.norm(got[1:3], axis=1), 1.0)
    with pytest.raises(ValueError):
        fibonacci_sphere(1, 0)


@pytest.fixture(scope="module")
def cenv():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_clutter_scene import make_env
    from mgs.env.clutter_table import ClutterTableEnv
    env = make_env()
    z = np.load(os.path.join(HERE, "golden", "clutter_scene.npz"))
    return ClutterTableEnv.from_dict({"gripper": env.gripper, "objects": env.objects,
                                      "env_state": {"state": z["state"]}})


def test_camera_frame(cenv):
    target = np.array([0.0, 0.0, -0.025])
    for i in range(4):
        cenv.update_camera_settings(4, i)
        E = cenv.get_camera_extrinsics()
        R, pos = E[:3, :3], E[:3, 3]
        assert E[3].tolist() == [0, 0, 0, 1] and pos[2] >= 0.01
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.linalg.det(R) == pytest.approx(1.0)
        # the optical axis (OpenCV z) passes through the target
        to = target - pos
        assert np.allclose(np.cross(R[:, 2], to), 0, atol=1e-12) and R[:, 2] @ to > 0
        # row 0 is the image top: image y (down) points below the horizon, image x is horizontal
        assert R[:, 1] @ [0, 0, 1.0] < 0 and abs(R[2, 0]) < 1e-12


def test_intrinsics_keep_the_reference_numbers(cenv):
    K = cenv.get_camera_intrinsics()
    assert K[0, 0] == pytest.approx(1206.5614781102, rel=1e-9) and K[1, 1] == pytest.approx(579.4112549695, rel=1e-9)
    assert K[0, 0] == pytest.approx(240 / np.tan(45 * np.pi / 720), rel=1e-12)
    assert K[1, 1] == pytest.approx(240 / np.tan(45 * np.pi / 360), rel=1e-12)
    assert K[0, 2] == 240 and K[1, 2] == 240 and K[2].tolist() == [0, 0, 1]
    Kr = cenv.get_render_intrinsics()
    assert Kr[0, 0] == Kr[1, 1] == K[1, 1]


def test_scan_scene_of_the_env(cenv):
    """table, origin marker and one mesh instance per object; the two foam
    bricks share a BVH; a removed object is not drawn; no random draw"""
    assert cenv.scan_geom_names == ["geom:table", "geom:base_origin", "obj0", "obj1", "obj2", "obj3", "obj4"]
    state = np.random.get_state()[1].copy()
    sc = cenv.scan_scene()
    assert np.array_equal(np.random.get_state()[1], state)
    assert sc.seg_id == [0, 1, 2, 3, 4, 5, 6] and len(sc.meshes) == 4 and sc.mesh[3] == sc.mesh[6]
    q = cenv.split_state(cenv.get_state())["qpos"]
    for k, (_, qs, _) in enumerate(cenv._obj_slices()):
        assert np.array_equal(sc.pos[2 + k], q[qs][:3])
        assert np.allclose(sc.rot[2 + k] @ sc.rot[2 + k].T, np.eye(3), atol=1e-12)
    cenv.removed.add("obj1")
    try:
        assert cenv.scan_scene().seg_id == [0, 1, 2, 4, 5, 6]
    finally:
        cenv.removed.discard("obj1")


def test_flat_colours(cenv):
    """objects and, without a colour in the scene dict, the table are 0.5 grey;
    a scene dict's table_rgba is kept through from_dict / to_dict"""
    from mgs.env.clutter_table import ClutterTableEnv
    c = cenv.scan_colors()
    assert c.shape == (7, 3) and np.all(c[0] == 0.5) and np.all(c[2:] == 0.5) and c[1].tolist() == [1, 0, 0]
    d = cenv.to_dict()
    assert "table_rgba" not in d["env_state"]
    d["env_state"]["table_rgba"] = [0.1, 0.2, 0.3, 1.0]
    env = ClutterTableEnv.from_dict(d)
    assert env.scan_colors()[0].tolist() == [0.1, 0.2, 0.3] and np.all(env.scan_colors()[2:] == 0.5)
    assert env.to_dict()["env_state"]["table_rgba"].tolist() == [0.1, 0.2, 0.3, 1.0]


# -- erosion ------------------------------------------------------------------
def test_erosion_is_cv2s():
    from scipy.ndimage import binary_erosion
    from mgs.scan.scene import erode_mask
    rng = np.random.default_rng(5)
    for p in (0.02, 0.1, 0.5):
        m = rng.random((3, 37, 29)) > p
        for it in (1, 5):
            want = np.stack([binary_erosion(x, structure=np.ones((3, 3)), iterations=it, border_value=1) for x in m])
            assert np.array_equal(T.erode(m, it), want)
            assert np.array_equal(erode_mask(m, it), want)
    assert np.array_equal(T.erode(m, 0), m) and np.array_equal(erode_mask(m, 0), m)


# -- host point-cloud processing ------------------------------------------------
def test_voxel_downsample():
    from mgs.util.img_proc import voxel_downsample_pcd
    p = np.array([[0.0, 0.0, 0.0], [0.4, 0.2, 0.1], [1.2, 0.0, 0.0], [0.1, 1.7, 0.0], [1.9, 0.3, 0.9], [0.0, 0.0, 1.5]])
    f = np.arange(12, dtype=np.float64).reshape(6, 2)
    P, F = voxel_downsample_pcd(p, f, 1.0)
    # voxels (x, y, z): (0,0,0) <- 0, 1; (0,0,1) <- 5; (0,1,0) <- 3; (1,0,0) <- 2, 4; raveled order x, y, z
    assert np.allclose(P, [[0.2, 0.1, 0.05], [0, 0, 1.5], [0.1, 1.7, 0], [1.55, 0.15, 0.45]])
    assert np.allclose(F, [[1, 2], [10, 11], [6, 7], [6, 7]])
    P32, F32 = voxel_downsample_pcd(p.astype(np.float32), f.astype(np.float32), 1.0)
    assert P32.dtype == np.float32 and F32.dtype == np.float32


def test_rgbd_to_pcd():
    from mgs.util.img_proc import rgbd_to_pcd
    rgbd = np.zeros((1, 2, 2, 4), np.float32)
    rgbd[0, ..., :3] = np.arange(12).reshape(2, 2, 3) / 12
    rgbd[0, ..., 3] = [[1.0, 2.0], [0.5, 4.0]]
    K = np.array([[2.0, 0, 1.0], [0, 4.0, 0.5], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]        # 90 degrees about z
    E[:3, 3] = [10, 20, 30]
    P, C = rgbd_to_pcd(rgbd, K, E[None])
    assert P.shape == (1, 2, 2, 3) and np.array_equal(C, rgbd[..., :3])
    for r in range(2):
        for c in range(2):
            z = float(rgbd[0, r, c, 3])
            cam = np.array([(c - 1.0) * z / 2.0, (r - 0.5) * z / 4.0, z])       # integer pixels, no half-pixel offset
            assert np.allclose(P[0, r, c], [10 - cam[1], 20 + cam[0], 30 + z])


# -- ABI ----------------------------------------------------------------------
def test_header_declares_the_scan_entries():
    from mgs.core import abi
    import ctypes
    txt = re.sub(r"/\*.*?\*/", "", open(abi.HEADER).read(), flags=re.S)
    for f in ("mgs_scan_render", "mgs_scan_points"):
        assert re.search(r"^int %s\(" % f, txt, re.M), f
    assert abi.MGS["MGS_ABI_VERSION"] == 24
    assert [n for n, _ in abi.ScanScene._fields_][:4] == ["ndraw", "nmesh", "nnode", "ntri"]
    assert ctypes.sizeof(abi.ScanScene) == 16 + 14 * ctypes.sizeof(ctypes.c_void_p)


def test_scene_packs_into_the_struct():
    from mgs.scan.scene import pack_scene
    a = T.small_scene().arrays()
    s, keep = pack_scene(a)
    assert (s.ndraw, s.nmesh, s.nnode, s.ntri) == (6, 3, len(a["node_skip"]), 413)
    assert s.draw_id[5] == 15 and s.tri_face[412] == 0 and s.mesh_node0[3] == s.nnode
    assert s.node_box[0] == a["node_box"][0, 0] and s.draw_rot[9 * 2 + 4] == a["draw_rot"][2, 1, 1]
