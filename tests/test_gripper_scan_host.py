"""The gripper scan on the host: the capsule and cylinder ray tests against a
sphere-tracing marcher and by hand, the numpy kinematics, the per-joint
segments and the scene arrays (tests/gripper_scan_truth.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gripper_scan_truth as G  # noqa: E402
import scan_truth as T  # noqa: E402

GRIPPERS = ("panda", "robotiq", "allegro", "shadow", "dexee")


def make_gripper(name):
    from mgs.gripper.allegro import GripperAllegro
    from mgs.gripper.dexee import GripperDexee
    from mgs.gripper.panda import GripperPanda
    from mgs.gripper.robotiq2f85 import GripperRobotiq2f85
    from mgs.gripper.shadow import GripperShadowRight
    from mgs.util.geo.transforms import SE3Pose
    cls = dict(panda=GripperPanda, robotiq=GripperRobotiq2f85, allegro=GripperAllegro, shadow=GripperShadowRight,
               dexee=GripperDexee)[name]
    return cls(SE3Pose(np.zeros(3), np.array([1.0, 0, 0, 0]), "wxyz"))


_ENVS = {}


def scan_env(name):
    from mgs.env.gripper_scan import GripperScanEnv
    if name not in _ENVS:
        _ENVS[name] = GripperScanEnv(make_gripper(name))
    return _ENVS[name]


# -- the ray tests ----------------------------------------------------------------
@pytest.mark.parametrize("cyl", [False, True], ids=["capsule", "cylinder"])
@pytest.mark.parametrize("r,h", [(0.009, 0.02), (0.0135, 0.015)])
def test_closed_form_against_sphere_tracing(cyl, r, h):
    """20 000 rays from the unit sphere toward the shape: where the march
    decides (hit: sdf < 1e-13; clear miss: smallest sdf > 1e-6), the closed
    form decides the same, and on hits |dt| <= 1e-9 (1 + t); at most 1 % of
    the rays (grazing ones) may stay undecided"""
    o, u = G.random_rays(20000, 1.5 * (r + h), seed=11 + int(cyl))
    sdf = (lambda p: G.sdf_cylinder(p, r, h)) if cyl else (lambda p: G.sdf_capsule(p, r, h))
    tm, smin = G.march(sdf, o, u)
    t = G.rod(o, u, r, h, cyl)
    hit, miss = np.isfinite(tm), ~np.isfinite(tm) & (smin > 1e-6)
    undecided = 1.0 - (hit | miss).mean()
    err = np.abs(t[hit] - tm[hit]) / (1.0 + tm[hit])
    print(f"cyl={cyl} r={r} h={h}: hits {hit.sum()}, clear misses {miss.sum()}, undecided {undecided:.4%}, "
          f"max |dt| / (1 + t) {err.max():.3g}")
    assert hit.sum() > 2000 and miss.sum() > 2000
    assert undecided <= 0.01
    assert np.all(np.isfinite(t[hit])) and not np.isfinite(t[miss]).any()
    assert err.max() <= 1e-9


def one(om, dm, r, h, cyl):
    return float(G.rod(np.array([om], np.float64), np.array([dm], np.float64), r, h, cyl)[0])


# a root from 1 m away: disc = B^2 - A C is rounded at the size of B^2 = 1 and s = sqrt(disc) is
# about r, so t = (-B - s) / A carries about 2^-53 / (2 r) = 1e-14; the exact cases below have none
TOL = 1e-13


def test_hand_cases():
    r, h = 0.009, 0.02
    # from the centre: the exit
    assert one([0, 0, 0], [0, 0, 1], r, h, False) == h + r
    assert one([0, 0, 0], [0, 0, 1], r, h, True) == h
    assert one([0, 0, 0], [0, 0, -2], r, h, True) == h / 2
    for cyl in (False, True):
        assert one([0, 0, 0], [1, 0, 0], r, h, cyl) == r                      # dm2 == 0, from inside
        assert one([-1, 0, 0.01], [1, 0, 0], r, h, cyl) == pytest.approx(1 - r, abs=TOL)   # dm2 == 0, from outside
        assert one([-1, 0, 0.01], [2, 0, 0], r, h, cyl) == pytest.approx((1 - r) / 2, abs=TOL)
        # axis-parallel (no side test): outside the radius a miss, inside the cap or the end sphere
        assert one([0.0091, 0, -1], [0, 0, 1], r, h, cyl) == np.inf
        assert one([0, -0.02, 1], [0, 0, -1], r, h, cyl) == np.inf
        assert one([-1, 0, 0], [-1, 0, 0], r, h, cyl) == np.inf                # behind the ray
    assert one([0.003, 0.004, -1], [0, 0, 1], r, h, True) == 1 - h
    assert one([0.003, 0.004, 1], [0, 0, -1], r, h, True) == 1 - h
    want = 1 - (h + np.sqrt(r * r - 0.005 ** 2))
    assert one([0.003, 0.004, -1], [0, 0, 1], r, h, False) == pytest.approx(want, abs=TOL)
    assert one([0.003, 0.004, 1], [0, 0, -1], r, h, False) == pytest.approx(want, abs=TOL)
    # beside the caps: the cylinder's rim is missed where the capsule's end sphere is hit
    assert one([-1, 0, h + 0.005], [1, 0, 0], r, h, True) == np.inf
    assert one([-1, 0, h + 0.005], [1, 0, 0], r, h, False) == pytest.approx(1 - np.sqrt(r * r - 0.005 ** 2), abs=TOL)
    # a cylinder of half-length 0 is a disc
    assert one([0.001, 0, -0.5], [0, 0, 1], r, 0.0, True) == 0.5


def test_capsule_of_zero_length_is_the_sphere_bitwise():
    """h = 0 in an unrotated frame: the end spheres' A, B, C are the sphere
    branch's a, b, c expression for expression (om = v, dm = d exactly, w = om2 -
    0), every root lies on one end's outer half, and a side root counts only at
    z == 0 exactly, where it is the sphere's own point: bitwise the same t"""
    from mgs.scan.scene import ScanScene
    pos = np.array([0.01, -0.02, 0.03])
    o, u = G.random_rays(5000, 0.06, seed=5)
    out = []
    for kind in ("sphere", "capsule"):
        sc = ScanScene()
        if kind == "sphere":
            sc.add_sphere(0, pos, 0.025)
        else:
            sc.add_capsule(0, pos, None, 0.025, 0.0)
        best = T._Best(len(o))
        assert G._primitive(sc.arrays(), 0, o, u * 1.7, best)
        out.append(best.t)
    assert np.isfinite(out[0]).sum() > 500 and (~np.isfinite(out[0])).sum() > 500
    assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64))
    inside = np.zeros((1, 3)) + pos + [0.001, 0.002, -0.003]                    # from inside: the exit
    for d in (u[:50] * 0.3):
        bs, bc = T._Best(1), T._Best(1)
        sc_s, sc_c = ScanScene(), ScanScene()
        sc_s.add_sphere(0, pos, 0.025)
        sc_c.add_capsule(0, pos, None, 0.025, 0.0)
        G._primitive(sc_s.arrays(), 0, inside, d[None], bs)
        G._primitive(sc_c.arrays(), 0, inside, d[None], bc)
        assert np.isfinite(bs.t[0]) and bs.t[0].tobytes() == bc.t[0].tobytes()


# -- kinematics -------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIPPERS)
def test_kinematics_at_qpos0(name):
    from mgs.scan.kin import body_poses
    cm = scan_env(name).model
    xpos, xquat = body_poses(cm, cm.qpos0)
    assert np.abs(xpos - cm.body_xpos0).max() <= 1e-12
    assert np.abs(xquat - cm.body_xquat0).max() <= 1e-12


def _by_type(cm, jtype):
    return [n for n, t in zip(cm.jnt_names, cm.jnt_type) if int(t) == jtype]


def test_panda_slide_translates_its_finger():
    from mgs.core.mjcf import quat2mat
    from mgs.scan.kin import body_poses, geom_poses, moved_geoms
    env = scan_env("panda")
    cm, q0 = env.model, env.qpos.copy()
    slides = _by_type(cm, 2)
    assert sorted(slides) == ["finger_joint1", "finger_joint2"]
    p0, R0 = geom_poses(cm, q0)
    for j in slides:
        jid = cm.jnt_names.index(j)
        q = q0.copy()
        q[cm.jnt_qposadr[jid]] += 0.013
        p1, R1 = geom_poses(cm, q)
        moved = moved_geoms(cm, j)
        assert 0 < len(moved) < len(p0)
        rest = np.setdiff1d(np.arange(len(p0)), moved)
        axis = quat2mat(body_poses(cm, q0)[1][cm.jnt_bodyid[jid]]) @ cm.jnt_axis[jid]
        assert np.abs((p1[moved] - p0[moved]) - 0.013 * axis).max() <= 1e-15
        assert np.array_equal(R1, R0) and np.array_equal(p1[rest], p0[rest])
    assert not set(moved_geoms(cm, slides[0])) & set(moved_geoms(cm, slides[1]))


def test_shadow_hinge_turns_what_it_moves():
    from mgs.core.mjcf import quat2mat
    from mgs.scan.kin import body_poses, geom_poses, moved_geoms
    env = scan_env("shadow")
    cm, q0 = env.model, env.qpos.copy()
    j, ang = "rh_FFJ3", 0.7
    jid = cm.jnt_names.index(j)
    assert int(cm.jnt_type[jid]) == 3
    q = q0.copy()
    q[cm.jnt_qposadr[jid]] += ang
    p0, R0 = geom_poses(cm, q0)
    p1, R1 = geom_poses(cm, q)
    changed = np.nonzero(np.any(p1 != p0, axis=1) | np.any(R1 != R0, axis=(1, 2)))[0]
    moved = moved_geoms(cm, j)
    assert np.array_equal(changed, moved) and len(moved) == 3       # proximal capsule, middle capsule, distal hull
    # rigid: distances within the moved set are kept
    d0 = np.linalg.norm(p0[moved][:, None] - p0[moved][None], axis=2)
    d1 = np.linalg.norm(p1[moved][:, None] - p1[moved][None], axis=2)
    assert np.abs(d1 - d0).max() <= 1e-12
    # about the world-frame axis through the anchor, which stays put
    b = int(cm.jnt_bodyid[jid])
    x0, xq0 = body_poses(cm, q0)
    x1, xq1 = body_poses(cm, q)
    anchor0 = x0[b] + quat2mat(xq0[b]) @ cm.jnt_pos[jid]
    anchor1 = x1[b] + quat2mat(xq1[b]) @ cm.jnt_pos[jid]
    assert np.abs(anchor1 - anchor0).max() <= 1e-12
    axis = quat2mat(xq0[b]) @ cm.jnt_axis[jid]
    Rw = T.rot(axis, ang)
    far = moved[-1]
    assert np.linalg.norm(p0[far] - anchor0) > 0.04
    assert np.abs((anchor0 + Rw @ (p0[far] - anchor0)) - p1[far]).max() <= 1e-12
    assert np.abs(Rw @ R0[far] - R1[far]).max() <= 1e-12


def test_free_joint_takes_pose_times_b2c():
    from mgs.scan.kin import body_poses
    from mgs.util.geo.transforms import SE3Pose
    env = scan_env("panda")
    cm = env.model
    a = cm.jnt_qposadr_by_name("freejoint")
    b2c = env.gripper.base_to_contact_transform()
    want = (SE3Pose(np.zeros(3), np.array([1.0, 0, 0, 0]), "wxyz") @ b2c).to_vec(layout="pq", type="wxyz")
    assert np.array_equal(env.qpos[a:a + 7], np.asarray(want, np.float64).reshape(-1))
    assert np.array_equal(env.qpos[a:a + 3], np.float32([0, 0, -0.102]).astype(np.float64))
    base = cm.jnt_bodyid[cm.jnt_names.index("freejoint")]
    xpos, xquat = body_poses(cm, env.qpos)
    assert np.array_equal(xpos[base], env.qpos[a:a + 3])
    assert np.abs(xquat[base] - env.qpos[a + 3:a + 7] / np.linalg.norm(env.qpos[a + 3:a + 7])).max() <= 1e-15
    # the quaternion is normalised, whatever the state holds
    q = env.qpos.copy()
    q[a + 3:a + 7] *= 3.0
    assert np.abs(body_poses(cm, q)[1] - xquat).max() <= 1e-15
    with pytest.raises(ValueError):
        body_poses(cm, q[:-1])


def test_state_and_joint_indices():
    env = scan_env("shadow")
    names = env.gripper.get_actuator_joint_names()
    idxs = env.get_joint_idxs(names)
    assert idxs == [env.model.jnt_qposadr_by_name(n) for n in names] and len(set(idxs)) == 22
    old = env.qpos.copy()
    try:
        env.set_qpos(np.arange(22) * 0.01, idxs)
        assert np.array_equal(env.qpos[idxs], np.arange(22) * 0.01)
        state = env.get_state()
        assert state.shape == (env.state_size(),)
        env.set_qpos(np.zeros(22), idxs)
        env.set_state(state)
        assert np.array_equal(env.qpos[idxs], np.arange(22) * 0.01)
        with pytest.raises(ValueError):
            env.set_state(state[:-1])
    finally:
        env.qpos = old


# -- segments -----------------------------------------------------------------------
def test_segments_of_the_shadow_hand():
    from mgs.scan.kin import moved_geoms
    env = scan_env("shadow")
    cm = env.model
    ng = len(cm.geom_bodyid)
    rng = np.random.default_rng(3)
    seg = rng.integers(-1, ng, size=(2, 24, 31)).astype(np.int32)
    keep = rng.random(seg.shape) < 0.7
    names, masks = env.segments(seg, keep)
    joints = [n for n, t in zip(cm.jnt_names, cm.jnt_type) if int(t) in (2, 3)]
    assert names == joints + ["body"] and len(joints) == 22
    assert masks.shape == (23,) + seg.shape and masks.dtype == bool
    assert not (masks & ~keep).any()                                    # never beyond image_masks
    body = masks[names.index("body")]
    assert np.array_equal(body, (seg != -1) & keep)
    assert np.array_equal(body, masks.any(axis=0))
    chain = [masks[names.index(f"rh_FFJ{k}")] for k in (4, 3, 2, 1)]
    sets = [set(moved_geoms(cm, f"rh_FFJ{k}")) for k in (4, 3, 2, 1)]
    assert [len(s) for s in sets] == [4, 3, 2, 1]
    for big, small, mb, ms in zip(sets, sets[1:], chain, chain[1:]):
        assert small < big                                              # strictly nested
        assert not (ms & ~mb).any() and (mb & ~ms).any()
    for k, n in enumerate(joints):
        assert np.array_equal(masks[k], np.isin(seg, moved_geoms(cm, n)) & keep)
    # an explicit mapping: segment name -> joint name
    names2, masks2 = env.segments(seg, keep, {"ff_j4": "rh_FFJ4", "thumb": "rh_THJ5"})
    assert names2 == ["ff_j4", "thumb"]
    assert np.array_equal(masks2[0], chain[0]) and np.array_equal(masks2[1], masks[names.index("rh_THJ5")])
    with pytest.raises(ValueError):
        env.segments(seg, keep, {"x": "no_such_joint"})


# -- scene arrays ---------------------------------------------------------------------
def test_add_capsule_and_cylinder_fill_the_arrays():
    from mgs.core import abi
    from mgs.scan.scene import ScanScene, pack_scene
    assert abi.MGS["MGS_SCAN_CAPSULE"] == G.CAPSULE == 3 and abi.MGS["MGS_SCAN_CYLINDER"] == G.CYLINDER == 4
    sc = ScanScene()
    R = T.rot([1, 2, 3], 0.4)
    assert sc.add_capsule(7, [0.1, 0.2, 0.3], R, 0.009, 0.02) == 0
    assert sc.add_cylinder(9, [0.0, 0.0, 0.1], None, 0.0135, 0.015) == 1
    S = sc.arrays()
    assert S["draw_type"].tolist() == [3, 4] and S["draw_id"].tolist() == [7, 9] and S["draw_mesh"].tolist() == [-1, -1]
    assert np.array_equal(S["draw_size"], [[0.009, 0.02, 0.0], [0.0135, 0.015, 0.0]])      # radius, half-length
    assert np.array_equal(S["draw_rot"][0], R) and np.array_equal(S["draw_rot"][1], np.eye(3))
    assert np.array_equal(S["draw_pos"], [[0.1, 0.2, 0.3], [0.0, 0.0, 0.1]])
    scene, keep = pack_scene(S)
    assert scene.ndraw == 2 and scene.nmesh == 0


def test_scan_scene_of_the_shadow_hand():
    from mgs.scan.kin import geom_poses
    env = scan_env("shadow")
    cm = env.model
    sc = env.scan_scene()
    S = sc.arrays()
    assert sc.ndraw == len(cm.geom_bodyid) == 36 and env.scan_geom_names == list(cm.geom_names)
    assert S["draw_id"].tolist() == list(range(36))
    counts = {k: int((S["draw_type"] == k).sum()) for k in range(5)}
    assert counts == {T.BOX: 11, T.SPHERE: 3, T.MESH: 5, G.CAPSULE: 10, G.CYLINDER: 7}
    assert len(sc.meshes) == 2                        # the four fingertips share one hull, the thumb has its own
    pos, rot = geom_poses(cm, env.qpos)
    assert np.array_equal(S["draw_pos"], pos)
    prim = S["draw_type"] != T.SPHERE
    assert np.array_equal(S["draw_rot"][prim], rot[prim])
    rods = np.isin(S["draw_type"], (G.CAPSULE, G.CYLINDER))
    assert np.array_equal(S["draw_size"][rods][:, :2], cm.geom_size[rods][:, :2]) and (S["draw_size"][rods] > 0)[:, :2].all()
    assert all(m.ntri >= 4 for m in sc.meshes)


def test_views_cover_the_sphere_and_need_two():
    env = scan_env("panda")
    with pytest.raises(ValueError):
        env.update_camera_settings(1, 0)
    from mgs.util.camera import fibonacci_sphere
    zs = []
    for i in range(6):
        env.update_camera_settings(6, i)
        E = env.get_camera_extrinsics()
        assert np.array_equal(E[:3, 3], fibonacci_sphere(6, i))              # not lifted
        assert np.abs(E[:3, 2] + E[:3, 3]).max() <= 1e-15                      # looks at the origin from distance 1
        assert np.abs(E[:3, :3].T @ E[:3, :3] - np.eye(3)).max() <= 1e-15
        zs.append(E[2, 3])
    assert min(zs) < -0.3 and max(zs) > 0.3
    env.scan_width, env.scan_height = 64, 48
    K, Kr = env.get_camera_intrinsics(), env.get_render_intrinsics()
    assert K[1, 1] == Kr[1, 1] == Kr[0, 0] == 24 / np.tan(45 * np.pi / 360)
    assert K[0, 0] == pytest.approx(24 / np.tan(45 * np.pi / 720)) and K[0, 2] == 32 and K[1, 2] == 24
