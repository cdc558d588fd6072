"""The gripper scan on the MI355X: capsule and cylinder drawables of
mgs_scan_kernel against the numpy truth of tests/gripper_scan_truth.py bit for
bit, the host check of their sizes, then GripperScanEnv (scan, segments, cloud)
and the scan_gripper CLI end to end."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_truth as C  # noqa: E402
import gripper_scan_truth as G  # noqa: E402
import scan_truth as T  # noqa: E402
from test_gripper_scan_host import make_gripper  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 44, 36      # no multiple of the 16 x 16 tile in either direction


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def render(S, pos, R, width, height):
    from mgs.core.engine import scan_render
    f = T.focal(height)
    return scan_render(S, pos, R, width, height, f, f, width / 2, height / 2)


def cameras(positions, target):
    from mgs.scan.scene import look_at_frame
    pos = np.asarray(positions, np.float64).reshape(-1, 3)
    R = []
    for p in pos:
        F = look_at_frame(p, target)
        R.append(np.stack([F[:, 0], -F[:, 1], -F[:, 2]], axis=1))
    return pos, np.array(R)


def forty_drawables():
    """a box, a sphere, SEVEN_TRIANGLES and 37 capsules and cylinders at random
    poses within 12 cm of the origin, radius and half-length log-uniform in
    1 mm .. 5 cm; drawable 20 is a capsule of half-length 0; drawables 31 and
    32 -- the last of the first staging group and the first of the second --
    are one capsule twice, ids 131 and 132.  Ids are 100 + index."""
    from mgs.scan.scene import ScanScene
    rng = np.random.default_rng(40)
    sc = ScanScene()
    sc.add_box(100, [0.05, -0.06, -0.08], T.rot([1, 1, 0], 0.5), [0.03, 0.02, 0.01])
    sc.add_sphere(101, [-0.07, 0.05, 0.02], 0.02)
    sc.add_mesh(102, [-0.04, -0.05, 0.06], T.rot([0, 1, 2], 1.0), *T.SEVEN_TRIANGLES)
    while sc.ndraw < 40:
        k = sc.ndraw
        pos, R = rng.uniform(-0.12, 0.12, 3), T.rot(rng.normal(size=3), rng.uniform(0, np.pi))
        r, h = np.exp(rng.uniform(np.log(0.001), np.log(0.05), 2))
        if k == 20:
            h = 0.0
        if k == 31:                     # the twins where the cameras see them
            pos, r, h = np.array([0.1, 0.12, -0.05]), 0.012, 0.03
        if k == 32:
            sc.add_capsule(100 + k, sc.pos[31], sc.rot[31], sc.size[31][0], sc.size[31][1])
        elif k == 31 or k == 20 or rng.random() < 0.5:
            sc.add_capsule(100 + k, pos, R, r, h)
        else:
            sc.add_cylinder(100 + k, pos, R, r, h)
    return sc


def check_parity(got, want):
    for k in ("seg", "tri", "ntest"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["depth"]), bits(want["depth"]))
    depth, seg, tri = want["brute"]
    assert np.array_equal(got["seg"], seg) and np.array_equal(got["tri"], tri)
    assert np.array_equal(bits(got["depth"]), bits(depth))


def test_primitive_parity():
    sc = forty_drawables()
    S = sc.arrays()
    assert sc.ndraw == 40 and set(S["draw_type"][32:]) == {G.CAPSULE, G.CYLINDER}
    assert S["draw_type"][20] == G.CAPSULE and S["draw_size"][20, 1] == 0.0
    pos, R = cameras([[0.45, 0.1, 0.2], [-0.3, -0.35, -0.15], [0.05, 0.4, -0.3]], [0.0, 0.0, 0.0])
    want = G.truth(S, pos, R, W, H)
    seen = set(np.unique(want["seg"]))
    assert {-1, 100, 101, 102, 120} <= seen and len(seen) > 25, "the truth first, on the CPU"
    types = S["draw_type"][want["seg"][want["seg"] >= 0] - 100]
    assert (types == G.CAPSULE).sum() > 200 and (types == G.CYLINDER).sum() > 200
    # the twin capsules: the lower drawable index wins every pixel they cover
    assert (want["seg"] == 131).sum() > 5 and not (want["seg"] == 132).any()
    got = render(S, pos, R, W, H)
    check_parity(got, want)
    assert not (got["seg"] == 132).any()
    # without the first twin the second takes exactly its pixels, at the same depths
    keep = np.arange(40) != 31
    S2 = dict(S, **{k: S[k][keep] for k in ("draw_type", "draw_id", "draw_mesh", "draw_pos", "draw_rot", "draw_size")})
    got2 = render(S2, pos, R, W, H)
    assert np.array_equal(got2["seg"] == 132, got["seg"] == 131)
    assert np.array_equal(bits(got2["depth"]), bits(got["depth"]))


@pytest.mark.parametrize("cyl", [True, False], ids=["cylinder", "capsule"])
def test_camera_inside_sees_the_exit(cyl):
    from mgs.scan.scene import ScanScene
    r, h = 0.05, 0.04
    sc = ScanScene()
    Rg, pg = T.rot([1, -2, 0.5], 0.8), np.array([0.01, 0.02, -0.03])
    (sc.add_cylinder if cyl else sc.add_capsule)(5, pg, Rg, r, h)
    S = sc.arrays()
    pos, R = cameras([pg + Rg @ [0.01, -0.02, 0.015]], pg + Rg @ [0.0, 0.05, 0.1])
    want = G.truth(S, pos, R, W, H)
    assert np.all(want["seg"] == 5) and np.all(want["depth"] > 0)
    got = render(S, pos, R, W, H)
    check_parity(got, want)
    # the hit points lie on the surface, seen from inside
    f = T.focal(H)
    o, d = T.camera_rays(pos, R, W, H, f, f, W / 2, H / 2)
    P = ((o + got["depth"].reshape(-1, 1) * d) - pg) @ Rg
    sdf = G.sdf_cylinder(P, r, h) if cyl else G.sdf_capsule(P, r, h)
    assert np.abs(sdf).max() <= 1e-9
    if cyl:
        assert (np.abs(np.abs(P[:, 2]) - h) < 1e-9).any() and (np.abs(np.hypot(P[:, 0], P[:, 1]) - r) < 1e-9).any()


def test_bad_sizes():
    from mgs.core import abi
    from mgs.core.engine import load_library
    from mgs.scan.scene import ScanScene, pack_scene
    L = load_library()
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    n = 4 * 4
    depth, seg, tri = np.full(n, 7.0), np.full(n, 7, np.int32), np.full(n, 7, np.int32)
    cp, cr = cameras([[0.0, 0.0, 0.5]], [0.0, 0.0, 0.0])

    def call(arrays):
        scene, keep = pack_scene(arrays)
        return L.mgs_scan_render(0, ctypes.byref(scene), 1, cp.ctypes.data_as(pd), cr.ctypes.data_as(pd), 4, 4, 5.0, 5.0,
                                 2.0, 2.0, depth.ctypes.data_as(pd), seg.ctypes.data_as(pi), tri.ctypes.data_as(pi),
                                 None, None)

    def scene(kind, r, h):
        sc = ScanScene()
        sc.add_box(0, [0.0, 0.0, -0.1], None, [0.5, 0.5, 0.01])
        (sc.add_capsule if kind == G.CAPSULE else sc.add_cylinder)(1, [0.0, 0.0, 0.0], None, r, h)
        return sc.arrays()
    for kind in (G.CAPSULE, G.CYLINDER):
        for r, h in ((0.0, 0.02), (np.nan, 0.02), (0.01, -0.001), (-0.01, 0.02), (np.inf, 0.02), (0.01, np.nan),
                     (0.01, np.inf)):
            assert call(scene(kind, r, h)) == abi.MGS["MGS_EINVAL"], (kind, r, h)
            msg = L.mgs_last_error()
            assert b"mgs_scan_render" in msg and b"drawable 1" in msg, msg
            assert np.all(depth == 7.0) and np.all(seg == 7) and np.all(tri == 7)      # nothing was written
    # box and sphere sizes are not checked, as before; an unknown type still is
    bad = scene(G.CAPSULE, 0.01, 0.02)
    bad["draw_type"][1] = 5
    assert call(bad) == abi.MGS["MGS_EINVAL"] and b"unknown drawable type" in L.mgs_last_error()
    assert np.all(seg == 7)
    # and a valid call works afterwards (half-length 0 is valid): a ball of 10 cm from 50 cm covers
    # the four inner pixels (slope 0.14 < 0.2), the box behind it the rest
    assert call(scene(G.CAPSULE, 0.1, 0.0)) == 0
    assert (seg.reshape(4, 4)[1:3, 1:3] == 1).all() and (seg == 0).sum() == 12 and np.all(depth != 7.0)


# -- the env ----------------------------------------------------------------------
def box_sdf(p, half):
    q = np.abs(p) - half
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)


def open_env(name):
    """the env at the open qpos of the gripper's config, as the CLI sets it"""
    from mgs.cli._hydra import compose
    from mgs.env.gripper_scan import GripperScanEnv
    cfg = compose("scan_gripper", ["gripper=" + {"robotiq": "robotiq_2f_85"}.get(name, name)])
    g = make_gripper(name)
    env = GripperScanEnv(g)
    env.set_qpos(np.array(cfg.qpos, np.float64), env.get_joint_idxs(g.get_actuator_joint_names()))
    return env


@pytest.fixture(scope="module")
def shadow():
    return open_env("shadow")


def check_scan(env, n, w, h):
    """scan n views and compare with the numpy truth on env.scan_scene(); the
    truth is the BVH walk alone: a sweep over every hull face of every pixel
    takes the CPU minutes, and test_primitive_parity holds walk and sweep together"""
    rgbd, extr, masks, seg = env.scan(num_images=n, width=w, height=h)
    assert rgbd.shape == (n, h, w, 4) and rgbd.dtype == np.float32 and extr.shape == (n, 4, 4)
    assert masks.shape == (n, h, w) and masks.dtype == bool and seg.shape == (n, h, w) and seg.dtype == np.int32
    S = env.scan_scene().arrays()
    K = env.get_render_intrinsics()
    o, d = T.camera_rays(extr[:, :3, 3], extr[:, :3, :3], w, h, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    depth, tseg, ttri, tntest = G.render_bvh(S, o, d, (n, h, w))
    res = env.last_scan
    assert np.array_equal(seg, tseg) and np.array_equal(res["tri"], ttri) and np.array_equal(res["ntest"], tntest)
    assert np.array_equal(bits(res["depth"]), bits(depth))
    assert np.array_equal(rgbd[..., 3], depth.astype(np.float32))
    assert np.all(rgbd[..., :3][seg != -1] == 0.5) and np.all(rgbd[seg == -1] == 0)
    assert np.array_equal(masks, T.erode(seg != -1, 5))
    # every hit pixel's point o + t d lies on the geom the pixel names
    hit = np.nonzero(seg.reshape(-1) != -1)[0]
    P, g, tri = o[hit] + depth.reshape(-1, 1)[hit] * d[hit], seg.reshape(-1)[hit], res["tri"].reshape(-1)[hit]
    cm = env.model
    worst = {}
    for k in np.unique(g):
        sel = g == k
        local = (P[sel] - S["draw_pos"][k]) @ S["draw_rot"][k]
        kind, size = int(S["draw_type"][k]), S["draw_size"][k]
        if kind == T.MESH:
            hid = int(cm.geom_hullid[k])
            verts = cm.hull_vert[cm.hull_vertadr[hid]:cm.hull_vertadr[hid] + cm.hull_vertnum[hid]]
            dist = T.point_tri_dist(local, verts[env._hull_faces[hid][tri[sel]]])
        else:
            assert np.all(tri[sel] == -1)
            dist = np.abs({T.BOX: lambda p: box_sdf(p, size), T.SPHERE: lambda p: np.linalg.norm(p, axis=1) - size[0],
                           G.CAPSULE: lambda p: G.sdf_capsule(p, size[0], size[1]),
                           G.CYLINDER: lambda p: G.sdf_cylinder(p, size[0], size[1])}[kind](local))
        worst[kind] = max(worst.get(kind, 0.0), float(dist.max()))
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-9, worst
    return seg, S


def test_env_scan_shadow(shadow):
    seg, S = check_scan(shadow, 4, 64, 64)
    won = np.bincount(S["draw_type"][seg[seg >= 0]], minlength=5)
    assert np.all(won > 0), won          # boxes, spheres, hulls, capsules and cylinders each win pixels at 64 x 64


def test_env_scan_robotiq():
    seg, S = check_scan(open_env("robotiq"), 4, 64, 64)
    won = np.bincount(S["draw_type"][seg[seg >= 0]], minlength=5)
    assert won[T.MESH] > 0 and won[T.BOX] > 0


def test_closing_a_joint_changes_only_its_segment(shadow):
    from mgs.scan.kin import moved_geoms
    env = shadow
    _, _, _, seg0 = env.scan(num_images=4, width=64, height=64)
    depth0 = env.last_scan["depth"]
    a = env.get_joint_idxs(["rh_FFJ3"])
    old = env.qpos.copy()
    try:
        env.set_qpos([0.9], a)
        _, _, _, seg1 = env.scan(num_images=4, width=64, height=64)
        depth1 = env.last_scan["depth"]
    finally:
        env.qpos = old
    moved = moved_geoms(env.model, "rh_FFJ3")
    changed = (seg0 != seg1) | (bits(depth0) != bits(depth1))
    silhouette = np.isin(seg0, moved) | np.isin(seg1, moved)
    assert changed.sum() > 10 and not (changed & ~silhouette).any()
    names, masks = env.segments(seg1, np.ones_like(changed))
    assert np.array_equal(masks[names.index("rh_FFJ3")], np.isin(seg1, moved))


def test_cloud(shadow):
    """4 views of 320 x 320 (the camera is 1 m away: at 64 x 64 the hand is a
    dozen pixels wide and five erosions leave nothing): the rows are the host chain on the same depth and
    seg -- scan_truth.points, compaction in (view, row, column) order, the
    farthest-point truth on the float32-rounded points"""
    env = shadow
    _, extr, masks, seg = env.scan(num_images=4, width=320, height=320)
    assert np.array_equal(masks, T.erode(seg != -1, 5)) and masks.sum() > 300
    region = np.array([-0.5, -0.5, 0.05, 0.5, 0.5, 0.5])
    P, geom, member = env.cloud(256, region)
    K = env.get_camera_intrinsics()
    tp, keep = T.points(env.last_scan["depth"], seg, extr, K[0, 0], K[1, 1], K[0, 2], K[1, 2], 5, region)
    print("eroded", masks.sum(), "kept", keep.sum())
    assert keep.sum() > 256 and keep.sum() < masks.sum(), "the region cuts the wrist off"
    pts32, g = tp[keep].astype(np.float32), seg[keep]
    idx = C.brute_fps(pts32.astype(np.float64), 256)
    assert P.dtype == np.float32 and P.shape == (256, 3) and np.array_equal(P, pts32[idx])
    assert geom.dtype == np.int32 and np.array_equal(geom, g[idx])
    names, _ = env.segments(seg, masks)
    assert member.shape == (len(names), 256) and member.dtype == bool and member[names.index("body")].all()
    from mgs.scan.kin import moved_geoms
    assert np.array_equal(member[names.index("rh_THJ4")], np.isin(geom, moved_geoms(env.model, "rh_THJ4")))
    assert np.all(P[:, 2] > 0.05)
    # with fewer kept points than asked for: every kept point, in compaction order; default region +-0.5 m
    P2, geom2, _ = env.cloud(100000)
    tp2, keep2 = T.points(env.last_scan["depth"], seg, extr, K[0, 0], K[1, 1], K[0, 2], K[1, 2], 5,
                          np.array([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]))
    assert np.array_equal(keep2, masks) and np.array_equal(P2, tp2[keep2].astype(np.float32))
    assert np.array_equal(geom2, seg[keep2])


def test_scan_gripper_cli(tmp_path, monkeypatch):
    from mgs.cli import scan_gripper
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path))
    scan_gripper.run(["gripper=shadow", "num_images=4", "width=64", "height=64", "num_points=128"])
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 1 and files[0].startswith("open_") and files[0].endswith(".npz")
    z = np.load(tmp_path / files[0], allow_pickle=False)
    nseg, ngeom = 23, 36
    want = dict(scans=((4, 64, 64, 4), np.float32), scan_extrinsics=((4, 4, 4), np.float64),
                scan_intrinsics=((3, 3), np.float64), scan_masks=((4, 64, 64), np.bool_),
                segments=((nseg, 4, 64, 64), np.bool_), segmentation=((4, 64, 64), np.int32))
    assert set(z.files) == set(want) | {"segment_names", "geom_names", "points", "point_geom", "point_segments"}
    for k, (shape, dt) in want.items():
        assert z[k].shape == shape and z[k].dtype == dt, k
    assert z["segment_names"].shape == (nseg,) and z["segment_names"].dtype.kind == "U"
    assert z["segment_names"][-1] == "body" and "rh_FFJ4" in z["segment_names"].tolist()
    assert z["geom_names"].shape == (ngeom,) and z["geom_names"].dtype.kind == "U"
    p = len(z["points"])
    assert p <= 128 and z["points"].shape == (p, 3) and z["points"].dtype == np.float32
    assert z["point_geom"].shape == (p,) and z["point_geom"].dtype == np.int32
    assert z["point_segments"].shape == (nseg, p) and z["point_segments"].dtype == np.bool_
    assert (z["segmentation"] >= 0).sum() > 100
    assert np.array_equal(z["segments"][-1], (z["segmentation"] != -1) & z["scan_masks"])
    assert z["scan_intrinsics"][1, 1] == 32 / np.tan(45 * np.pi / 360)
