"""The posed gripper cloud on the host: the kinematic trees
(mgs/sampler/kin/tree.py) and the numpy restatement of the kernel
(tests/pose_truth.py) against the reference as written and against the
independent host kinematics of mgs/scan/kin.py.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pose_truth as PT  # noqa: E402
from test_gripper_scan_host import GRIPPERS, scan_env  # noqa: E402

# 1e-12 m: the reference's sequential masked transforms against the single
# composite transform measure 1.2e-15 m on the unit-quaternion Shadow table
# (each is a handful of f64 products of O(1) quantities at 0.3 m); the bound
# leaves three orders for other joint values.  The same bound holds the tree of
# a compiled model against mgs.scan.kin.geom_poses (chains of <= 5 joints).
TOL = 1e-12


def shadow_tree():
    from mgs.sampler.kin.model import ShadowKinematicsModel
    from mgs.sampler.kin.tree import tree_from_kinematics
    kin = ShadowKinematicsModel()
    return kin, tree_from_kinematics(kin)


def nested_masks(tree, link):
    """the reference's representation of `link`: row j holds the points joint j moves"""
    masks = np.zeros((tree.nlink, len(link)), bool)
    for p, l in enumerate(link):
        a = int(l) - 1
        while a >= 0:
            masks[a, p] = True
            a = int(tree.parent[a])
    return masks


# -- the Shadow table ------------------------------------------------------------------
def test_table_quaternions_are_normalised_at_build():
    kin, tree = shadow_tree()
    raw = np.abs(np.linalg.norm(kin.kin_tf[:, :4], axis=1) - 1.0).max()
    unit = np.abs(np.linalg.norm(tree.kin_tf[:, :4], axis=1) - 1.0).max()
    print(f"table quaternions off unit length by {raw:.3g}, the tree's by {unit:.3g}")
    assert 1e-7 < raw < 1e-6 and unit <= 2.3e-16
    assert np.array_equal(tree.parent, kin.parents()) and tree.nlink == kin.num_dofs
    assert np.array_equal(tree.kin_tf[:, 4:], kin.kin_tf[:, 4:]) and np.array_equal(tree.joint_tf, kin.joint_tf)


def test_kernel_form_equals_the_reference_on_the_shadow_table():
    kin, tree = shadow_tree()
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.3, 0.3, (500, 3))
    link = rng.integers(0, tree.nlink + 1, 500).astype(np.int32)
    link[:tree.nlink + 1] = np.arange(tree.nlink + 1)
    masks = nested_masks(tree, link)
    worst = 0.0
    for _ in range(3):
        theta = rng.uniform(kin.joint_ranges[:, 0], kin.joint_ranges[:, 1])
        got, _ = PT.pose_kernel(tree, pts, link, theta[None])
        want = PT.pose_reference(kin.chains, tree.kin_tf, tree.joint_tf, pts, theta, masks)
        worst = max(worst, np.abs(got[0] - want).max())
        assert np.abs(got[0][link > 0] - pts[link > 0]).max() > 1e-3      # the points do move
    print(f"pose_kernel against pose_reference: {worst:.3g} m")
    assert worst <= TOL


def test_links_from_segments_inverts_the_masks():
    _, tree = shadow_tree()
    rng = np.random.default_rng(6)
    link = rng.integers(0, tree.nlink + 1, 300).astype(np.int32)
    masks = nested_masks(tree, link)
    assert np.array_equal(tree.links_from_segments(masks), link)
    order = list(rng.permutation(tree.nlink))
    assert np.array_equal(tree.links_from_segments(masks[order], [tree.joint_names[i] for i in order]), link)
    p = int(np.nonzero(link == 4)[0][0])      # the first finger's tip: dofs 0 .. 3
    broken = masks.copy()
    broken[1, p] = False
    with pytest.raises(ValueError, match="ancestors"):
        tree.links_from_segments(broken)
    extra = masks.copy()
    extra[9, p] = True                        # a joint of another finger
    with pytest.raises(ValueError, match="ancestors"):
        tree.links_from_segments(extra)


def test_theta_scan_gives_the_scan_back():
    kin, tree = shadow_tree()
    rng = np.random.default_rng(7)
    tree.theta_scan = rng.uniform(kin.joint_ranges[:, 0], kin.joint_ranges[:, 1])
    pts = rng.uniform(-0.3, 0.3, (200, 3))
    link = rng.integers(0, tree.nlink + 1, 200).astype(np.int32)
    got, _ = PT.pose_kernel(tree, pts, link, tree.theta_scan[None])
    print(f"theta = theta_scan: {np.abs(got[0] - pts).max():.3g} m")
    assert np.abs(got[0] - pts).max() <= 1e-14
    base = link == 0
    assert base.any() and np.array_equal(got[0][base].view(np.int64), pts[base].view(np.int64))
    other, _ = PT.pose_kernel(tree, pts, link, rng.uniform(kin.joint_ranges[:, 0], kin.joint_ranges[:, 1])[None])
    assert np.array_equal(other[0][base].view(np.int64), pts[base].view(np.int64))


# -- compiled models -------------------------------------------------------------------
def random_qpos(cm, env, rng):
    """the env's free-joint pose and every hinge / slide joint inside its range"""
    from mgs.scan import kin
    q = env.qpos.copy()
    for j, t in enumerate(cm.jnt_type):
        if int(t) in (kin.SLIDE, kin.HINGE):
            lo, hi = cm.jnt_range[j] if int(cm.jnt_limited[j]) else (-0.5, 0.5)
            q[int(cm.jnt_qposadr[j])] = rng.uniform(lo, hi)
    return q


def geom_truth(cm, qA, qB, geom, pts):
    """G_g(q_B) . G_g(q_A)^-1 . p by mgs.scan.kin.geom_poses (independent code)"""
    from mgs.scan import kin
    pA, RA = kin.geom_poses(cm, qA)
    pB, RB = kin.geom_poses(cm, qB)
    local = np.einsum("pji,pj->pi", RA[geom], pts - pA[geom])
    return pB[geom] + np.einsum("pij,pj->pi", RB[geom], local)


@pytest.mark.parametrize("name", GRIPPERS)
def test_tree_of_a_model_against_geom_poses(name):
    from mgs.sampler.kin.tree import tree_from_model
    from mgs.scan import kin
    env = scan_env(name)
    cm = env.model
    rng = np.random.default_rng(GRIPPERS.index(name))
    ng = len(cm.geom_bodyid)
    geom = np.repeat(np.arange(ng), 5)
    local = rng.uniform(-0.02, 0.02, (len(geom), 3))
    states = [random_qpos(cm, env, rng) for _ in range(3)]
    worst = 0.0
    for a in range(3):
        qA, qB = states[a], states[(a + 1) % 3]
        pA, RA = kin.geom_poses(cm, qA)
        pts = pA[geom] + np.einsum("pij,pj->pi", RA[geom], local)
        tree = tree_from_model(cm, qA)
        assert np.array_equal(tree.theta_scan, tree.theta_from_qpos(qA))
        link = tree.link_of_geoms(cm)[geom]
        assert link.min() == 0 and link.max() == tree.nlink
        got, _ = PT.pose_kernel(tree, pts, link, tree.theta_from_qpos(qB)[None])
        want = geom_truth(cm, qA, qB, geom, pts)
        assert np.abs(want - pts).max() > 1e-3
        worst = max(worst, np.abs(got[0] - want).max())
    print(f"{name}: pose_kernel against geom_poses {worst:.3g} m over {tree.nlink} links")
    assert worst <= TOL


def test_panda_slides_take_the_zero_axis_branch():
    env = scan_env("panda")
    tree = env.kinematic_tree()
    assert tree.joint_names == ["finger_joint1", "finger_joint2"] and list(tree.parent) == [-1, -1]
    assert np.all(tree.joint_tf[:, 3:] == 0.0)                       # no revolute axis: norm 0
    assert np.all(np.linalg.norm(tree.joint_tf[:, :3], axis=1) > 0.99)
    for th in (0.0, 0.013, -0.02):
        J = PT.joint_tf(tree.joint_tf[0], th)
        assert np.array_equal(J[:4], [1.0, 0.0, 0.0, 0.0]) and np.array_equal(J[4:], tree.joint_tf[0, :3] * th)
    # a finger's point moves by the slide along the finger's axis in the world, nothing else
    pts = np.array([[0.01, 0.02, 0.03]])
    got, links = PT.pose_kernel(tree, pts, [1], tree.theta_scan[None] + np.array([[0.01, 0.0]]))
    step = got[0, 0] - pts[0]
    assert abs(np.linalg.norm(step) - 0.01) <= 1e-15
    from mgs.core.mjcf import quat2mat
    axis = quat2mat(tree.kin_tf[0, :4]) @ tree.joint_tf[0, :3]
    assert np.abs(step - 0.01 * axis).max() <= 1e-15


def test_parents_stated_by_hand():
    rq = scan_env("robotiq").kinematic_tree()
    par = dict(zip(rq.joint_names, rq.parent))
    idx = {n: i for i, n in enumerate(rq.joint_names)}
    # the driver and the spring link hang from `base`, a body without a joint under the free joint's body
    assert par["right_driver_joint"] == -1 and par["right_spring_link_joint"] == -1
    assert par["right_coupler_joint"] == idx["right_driver_joint"]
    assert par["right_follower_joint"] == idx["right_spring_link_joint"]     # the spanning tree, not the loop
    assert par["left_follower_joint"] == idx["left_spring_link_joint"]
    cm = scan_env("robotiq").model
    link = rq.link_of_geoms(cm)
    for g, b in enumerate(cm.geom_bodyid):      # the pads: bodies without a joint below the follower
        if cm.body_names[int(b)] in ("right_pad", "right_silicone_pad"):
            assert link[g] == idx["right_follower_joint"] + 1
        if cm.body_names[int(b)] in ("base_mount", "base"):
            assert link[g] == 0
    sh = scan_env("shadow").kinematic_tree()
    par = dict(zip(sh.joint_names, sh.parent))
    idx = {n: i for i, n in enumerate(sh.joint_names)}
    # rh_palm has no joint: the knuckles hang from the base
    assert par["rh_FFJ4"] == -1 and par["rh_THJ5"] == -1 and par["rh_LFJ5"] == -1
    assert par["rh_FFJ3"] == idx["rh_FFJ4"] and par["rh_LFJ4"] == idx["rh_LFJ5"] and par["rh_THJ1"] == idx["rh_THJ2"]
    assert sh.nlink == 22 and "rh_WRJ1" not in sh.joint_names


TWO_JOINT_XML = """
<mujoco>
  <compiler angle="radian" autolimits="true"/>
  <option integrator="implicitfast" timestep="0.001" cone="elliptic" gravity="0 0 0"/>
  <worldbody>
    <body name="root" pos="0.1 0 0.2" quat="0.8 0.6 0 0">
      <joint name="freejoint" type="free"/>
      <geom name="g_root" type="sphere" size="0.01"/>
      <body name="a" pos="0.02 0 0.01" quat="0.6 0 0.8 0">
        <joint name="a_hinge" type="hinge" axis="0 0.6 0.8" pos="0.01 0 0" range="-1 1"/>
        <geom name="g_a" type="box" size="0.01 0.01 0.01"/>
        <body name="m" pos="0 0.03 0">
          <geom name="g_m" type="sphere" size="0.01" pos="0.01 0 0"/>
          <body name="c" pos="0 0 0.04" quat="0.6 0.8 0 0">
            <joint name="c_hinge" type="hinge" axis="1 0 0" pos="0 0.01 0.02" range="-1 1"/>
            <joint name="c_slide" type="slide" axis="0 0.8 0.6" pos="0.03 0 0" range="-0.02 0.02"/>
            <geom name="g_c" type="capsule" size="0.005 0.02" pos="0 0.01 0" quat="0.8 0 0.6 0"/>
          </body>
        </body>
      </body>
    </body>
    <body name="thing" pos="0 0 1">
      <joint name="thing_free" type="free"/>
      <geom name="g_thing" type="box" size="0.02 0.02 0.02"/>
      <body name="thing_lid" pos="0 0 0.03">
        <joint name="lid_hinge" type="hinge" axis="0 0 1" range="-1 1"/>
        <geom name="g_lid" type="sphere" size="0.01"/>
      </body>
    </body>
  </worldbody>
</mujoco>
"""


def test_two_joints_on_a_body_a_jointless_body_between_and_a_foreign_free_joint():
    from mgs.core.mjcf import compile_xml
    from mgs.sampler.kin.tree import tree_from_model
    cm = compile_xml(TWO_JOINT_XML, {})
    tree = tree_from_model(cm)
    assert tree.joint_names == ["a_hinge", "c_hinge", "c_slide"]       # not the object's lid
    assert list(tree.parent) == [-1, 0, 1]                              # over body m; then the same body
    assert np.all(tree.joint_tf[[0, 1], :3] == 0) and np.all(tree.joint_tf[2, 3:] == 0)
    assert np.array_equal(tree.joint_tf[2, :3], cm.jnt_axis[cm.jnt_names.index("c_slide")])
    names = list(cm.geom_names)
    link = tree.link_of_geoms(cm)
    assert [int(link[names.index(n)]) for n in ("g_root", "g_a", "g_m", "g_c", "g_lid")] == [0, 1, 1, 3, 0]
    rng = np.random.default_rng(3)
    adr = {n: int(cm.jnt_qposadr[cm.jnt_names.index(n)]) for n in tree.joint_names}
    qA, qB = cm.qpos0.copy(), cm.qpos0.copy()
    for q in (qA, qB):
        q[adr["a_hinge"]], q[adr["c_hinge"]], q[adr["c_slide"]] = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.02, 0.02)
    geom = np.repeat([names.index(n) for n in ("g_root", "g_a", "g_m", "g_c")], 5)
    from mgs.scan import kin
    pA, RA = kin.geom_poses(cm, qA)
    pts = pA[geom] + np.einsum("pij,pj->pi", RA[geom], rng.uniform(-0.02, 0.02, (len(geom), 3)))
    tree = tree_from_model(cm, qA)
    got, _ = PT.pose_kernel(tree, pts, link[geom], tree.theta_from_qpos(qB)[None])
    err = np.abs(got[0] - geom_truth(cm, qA, qB, geom, pts)).max()
    print(f"two joints on a body: {err:.3g} m")
    assert err <= TOL


def test_theta_from_named_leaves_the_other_joints_at_rest():
    env = scan_env("allegro")
    tree = env.kinematic_tree()
    vals = np.array([[0.3, -0.1], [0.2, 0.4]])
    th = tree.theta_from_named(vals, ["thj1", "ffj0"])
    assert th.shape == (2, tree.nlink)
    i, j = tree.joint_names.index("thj1"), tree.joint_names.index("ffj0")
    assert np.array_equal(th[:, i], vals[:, 0] - tree.qpos0[i]) and np.array_equal(th[:, j], vals[:, 1] - tree.qpos0[j])
    rest = np.ones(tree.nlink, bool)
    rest[[i, j]] = False
    assert np.all(th[:, rest] == 0.0)
    with pytest.raises(ValueError, match="unknown joint"):
        tree.theta_from_named(vals, ["thj1", "nope"])


def test_a_tree_refuses_a_forward_parent():
    from mgs.sampler.kin.tree import KinematicTree
    eye = np.tile([1.0, 0, 0, 0, 0, 0, 0], (2, 1))
    with pytest.raises(ValueError, match="parent"):
        KinematicTree(parent=[1, -1], kin_tf=eye, joint_tf=np.zeros((2, 6)), joint_names=["a", "b"], theta_scan=np.zeros(2))


def test_get_kinematics_still_knows_the_shadow_hand_only():
    from mgs.sampler.kin.model import get_kinematics
    assert get_kinematics("ShadowHand").name == "ShadowHand"
    with pytest.raises(ValueError):
        get_kinematics("Panda")


# -- the header mirror -----------------------------------------------------------------
def test_pose_tree_mirror_matches_the_header():
    from mgs.core import abi
    txt = open(abi.HEADER).read()
    body = txt[txt.index("typedef struct mgs_pose_tree"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("} mgs_pose_tree;")], flags=re.S)
    names = re.findall(r"(?:int32_t|double)\s+(\w+)(?:\[\w+\])*\s*;", body)
    assert [f for f, _ in abi.PoseTree._fields_] == names == ["nlink", "parent", "kin_tf", "joint_tf", "theta_scan"]
    n = abi.MGS["MGS_POSE_MAXLINK"]
    assert n == 32
    # int32 nlink + parent[32], padded to 8, then 7 + 6 + 1 doubles per link
    assert ctypes.sizeof(abi.PoseTree) == (4 * (1 + n) + 4) + 8 * n * (7 + 6 + 1)
    assert abi.PoseTree.kin_tf.offset == 4 * (1 + n) + 4
    _, tree = shadow_tree()
    T = abi.make_pose_tree(tree)
    assert T.nlink == tree.nlink and list(T.parent)[:tree.nlink] == list(tree.parent)
    assert np.array_equal(np.ctypeslib.as_array(T.kin_tf)[:tree.nlink], tree.kin_tf)
    assert np.array_equal(np.ctypeslib.as_array(T.joint_tf)[:tree.nlink], tree.joint_tf)
