"""The posed gripper cloud on the MI355X (csrc/mgs_pose.hip through the C-ABI):
bit-exact parity with the numpy restatement of the kernel (tests/pose_truth.py)
at the smallest shapes that reach every edge, the host refusals, the
device-pointer entry, and the scan -> pose chain of GripperScanEnv and the
pose_gripper_cloud CLI against the independent host kinematics."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pose_truth as PT  # noqa: E402
from test_gripper_scan_host import make_gripper  # noqa: E402
from test_pose_host import TOL, geom_truth, random_qpos  # noqa: E402

pytestmark = pytest.mark.gpu

# the scan of the end-to-end tests: 4 views of SCAN_SIZE x SCAN_SIZE.  The camera
# is 1 m away and cloud() erodes the masks five times, so a small image leaves no
# point at all (measured: Allegro 0 points at 48 and 64, 3 at 96, 51 on one geom
# at 128; Panda 0 up to 96); at 320 -- the size tests/test_gripper_scan_gpu.py
# takes its cloud at -- 256 points lie on 19 Allegro geoms and 4 Panda geoms.
SCAN_SIZE = 320


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def shadow_case(seed=0):
    """the Shadow table scanned at a random joint state: 70 points, some on every
    link and on the base except link 10 (dof 9), which has none; 3 joint states"""
    from mgs.sampler.kin.model import ShadowKinematicsModel
    from mgs.sampler.kin.tree import tree_from_kinematics
    kin = ShadowKinematicsModel()
    rng = np.random.default_rng(seed)
    lo, hi = kin.joint_ranges[:, 0], kin.joint_ranges[:, 1]
    tree = tree_from_kinematics(kin, theta_scan=rng.uniform(lo, hi))
    link = (np.arange(70) % (tree.nlink + 1)).astype(np.int32)
    link[link == 10] = 0
    link = rng.permutation(link)
    pts = rng.uniform(-0.3, 0.3, (70, 3))
    theta = rng.uniform(lo, hi, (3, tree.nlink))
    poses = np.stack([random_pose(rng) for _ in range(3)])
    return tree, pts, link, theta, poses


def random_pose(rng):
    q = rng.normal(size=4)
    H = np.eye(4)
    H[:3, :3] = PT.quat2mat(q / np.linalg.norm(q))
    H[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    return H


_TRUTH = {}


def shadow_truth(with_base):
    """pose_kernel of shadow_case, computed once"""
    if with_base not in _TRUTH:
        tree, pts, link, theta, poses = shadow_case()
        _TRUTH[with_base] = PT.pose_kernel(tree, pts, link, theta, poses if with_base else None)
    return _TRUTH[with_base]


def check_exact(res, want_pts, want_links, dtype):
    want = want_pts if dtype == np.float64 else want_pts.astype(np.float32)
    assert res["points"].dtype == dtype and res["points"].shape == want.shape
    assert np.array_equal(bits(res["points"]), bits(want))
    assert np.array_equal(bits(res["links"]), bits(want_links))


@pytest.mark.parametrize("with_base", [False, True], ids=["scan-frame", "placed"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_parity_two_groups_the_second_ragged(with_base, dtype):
    from mgs.core.engine import pose_cloud
    tree, pts, link, theta, poses = shadow_case()
    assert set(link) == set(range(tree.nlink + 1)) - {10}
    want, wlinks = shadow_truth(with_base)
    res = pose_cloud(tree, pts, link, theta, base=poses if with_base else None, dtype=dtype, points_per_group=64)
    check_exact(res, want, wlinks, dtype)
    if not with_base:       # the base's points leave the kernel as they came
        for b in range(3):
            assert np.array_equal(bits(res["points"][b][link == 0]), bits(pts[link == 0].astype(dtype)))
    print(f"kernel {res['kernel_ms']:.3f} ms")


def test_one_point():
    from mgs.core.engine import pose_cloud
    tree, pts, link, theta, poses = shadow_case()
    p = int(np.nonzero(link == 22)[0][0])
    want, wlinks = PT.pose_kernel(tree, pts[p:p + 1], link[p:p + 1], theta, poses)
    for dtype in (np.float64, np.float32):
        check_exact(pose_cloud(tree, pts[p:p + 1], link[p:p + 1], theta, base=poses, dtype=dtype), want, wlinks, dtype)


def test_one_state_1025_points_on_auto_grouping():
    """B = 1: the host spreads the points over groups of one tile; 1025 = four tiles and one point"""
    from mgs.core.engine import pose_cloud
    tree, _, _, theta, _ = shadow_case()
    rng = np.random.default_rng(1)
    pts = rng.uniform(-0.3, 0.3, (1025, 3))
    link = rng.integers(0, tree.nlink + 1, 1025).astype(np.int32)
    want, wlinks = PT.pose_kernel(tree, pts, link, theta[:1])
    for dtype in (np.float64, np.float32):
        check_exact(pose_cloud(tree, pts, link, theta[:1], dtype=dtype), want, wlinks, dtype)
    # an explicit group of several tiles with a ragged last one gives the same
    check_exact(pose_cloud(tree, pts, link, theta[:1], dtype=np.float32, points_per_group=600), want, wlinks, np.float32)


def chain_tree(seed=2):
    """32 links: four chains of depth 8, hinges (axes of any length) and slides alternating"""
    from mgs.sampler.kin.tree import KinematicTree
    rng = np.random.default_rng(seed)
    n = 32
    parent = np.array([-1 if i % 8 == 0 else i - 1 for i in range(n)], np.int32)
    q = rng.normal(size=(n, 4))
    kin_tf = np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(-0.05, 0.05, (n, 3))], axis=1)
    joint_tf = np.zeros((n, 6))
    v = rng.normal(size=(n, 3))
    hinge = (np.arange(n) % 2 == 0) ^ (np.arange(n) // 8 % 2 == 1)
    joint_tf[hinge, 3:] = v[hinge] * rng.uniform(0.5, 2.0, (hinge.sum(), 1))
    joint_tf[~hinge, :3] = v[~hinge] / np.linalg.norm(v[~hinge], axis=1, keepdims=True)
    return KinematicTree(parent=parent, kin_tf=kin_tf, joint_tf=joint_tf, joint_names=[f"j{i}" for i in range(n)],
                         theta_scan=rng.uniform(-1.0, 1.0, n))


def test_thirty_two_links():
    from mgs.core.engine import pose_cloud
    tree = chain_tree()
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.3, 0.3, (99, 3))
    link = (np.arange(99) % 33).astype(np.int32)
    theta = rng.uniform(-1.5, 1.5, (2, 32))
    poses = np.stack([random_pose(rng) for _ in range(2)])
    want, wlinks = PT.pose_kernel(tree, pts, link, theta, poses)
    check_exact(pose_cloud(tree, pts, link, theta, base=poses, dtype=np.float64, points_per_group=64), want, wlinks,
                np.float64)
    check_exact(pose_cloud(tree, pts, link, theta, base=poses, dtype=np.float32), want, wlinks, np.float32)


def test_tree_size():
    from mgs.core import abi
    from mgs.core.engine import load_library
    assert load_library().mgs_pose_tree_size() == ctypes.sizeof(abi.PoseTree)


def test_host_refusals_launch_nothing():
    from mgs.core import abi
    from mgs.core.engine import load_library, pose_cloud
    L = load_library()
    tree, pts, link, theta, _ = shadow_case()
    d = ctypes.c_double

    def call(T, lk, nl):
        out = np.full((3, 70, 3), 7.0)
        links = np.full((3, nl, 7), 7.0)
        th = np.zeros((3, nl))
        rc = L.mgs_pose_cloud(0, ctypes.byref(T), 70, abi.ptr(pts, d), abi.ptr(lk, ctypes.c_int32), 3, abi.ptr(th, d),
                              None, 0, out.ctypes.data_as(ctypes.c_void_p), abi.ptr(links, d), 64, None)
        assert np.all(out == 7.0) and np.all(links == 7.0)
        return rc, L.mgs_last_error()

    EINVAL = abi.MGS["MGS_EINVAL"]
    bad_link = link.copy()
    bad_link[5] = tree.nlink + 1
    rc, msg = call(abi.make_pose_tree(tree), bad_link, tree.nlink)
    assert rc == EINVAL and b"point_link" in msg
    neg_link = link.copy()
    neg_link[69] = -1
    assert call(abi.make_pose_tree(tree), neg_link, tree.nlink)[0] == EINVAL
    T = abi.make_pose_tree(tree)
    T.parent[4] = 4
    rc, msg = call(T, link, tree.nlink)
    assert rc == EINVAL and b"parent" in msg
    T = abi.make_pose_tree(tree)
    T.nlink = 33
    rc, msg = call(T, link, 33)
    assert rc == EINVAL and b"nlink" in msg
    T.nlink = 0
    assert call(T, link, 1)[0] == EINVAL
    # nothing to do: MGS_OK without a launch
    out = np.full(3, 7.0)
    assert L.mgs_pose_cloud(0, ctypes.byref(abi.make_pose_tree(tree)), 0, None, None, 3, abi.ptr(theta, d), None, 0,
                            out.ctypes.data_as(ctypes.c_void_p), None, 0, None) == 0 and np.all(out == 7.0)
    assert L.mgs_pose_cloud(0, ctypes.byref(abi.make_pose_tree(tree)), 70, abi.ptr(pts, d),
                            abi.ptr(link, ctypes.c_int32), 0, None, None, 0, None, None, 0, None) == 0
    # and the next valid call is exact
    want, wlinks = shadow_truth(False)
    check_exact(pose_cloud(tree, pts, link, theta, dtype=np.float64, points_per_group=64), want, wlinks, np.float64)


def test_device_pointer_entry():
    import torch
    from mgs.core.engine import pose_cloud, pose_cloud_torch
    tree, pts, link, theta, poses = shadow_case()
    dev = torch.device("cuda", 0)
    tx, tl = torch.from_numpy(pts).to(dev), torch.from_numpy(link).to(dev)
    tth, tb = torch.from_numpy(theta).to(dev), torch.from_numpy(poses).to(dev)
    for dtype, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        for base, tbase in ((None, None), (poses, tb)):
            host = pose_cloud(tree, pts, link, theta, base=base, dtype=dtype, points_per_group=64)
            res = pose_cloud_torch(tree, tx, tl, tth, base=tbase, dtype=tdt, points_per_group=64)
            assert res["points"].device == dev and res["points"].dtype == tdt
            torch.cuda.synchronize(dev)
            assert np.array_equal(bits(res["points"].cpu().numpy()), bits(host["points"]))
            assert np.array_equal(bits(res["links"].cpu().numpy()), bits(host["links"]))
    # into a given tensor, on another stream
    out = torch.empty((3, 70, 3), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        res = pose_cloud_torch(tree, tx, tl, tth, base=tb, out=out)
    s.synchronize()
    assert res["points"].data_ptr() == out.data_ptr()
    assert np.array_equal(bits(out.cpu().numpy()), bits(shadow_truth(True)[0].astype(np.float32)))


# -- scan -> pose ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["allegro", "panda"])
def test_scan_then_pose(name):
    from mgs.env.gripper_scan import GripperScanEnv
    env = GripperScanEnv(make_gripper(name))
    cm = env.model
    rng = np.random.default_rng(11)
    qA = random_qpos(cm, env, rng)
    env.qpos = qA.copy()
    env.scan(num_images=4, width=SCAN_SIZE, height=SCAN_SIZE)
    pts, geom, _ = env.cloud(256)
    print(f"{name}: {len(pts)} points at {SCAN_SIZE} x {SCAN_SIZE}")
    assert len(pts) > 0
    tree = env.kinematic_tree()
    qB = [random_qpos(cm, env, rng) for _ in range(2)]
    theta = np.stack([tree.theta_from_qpos(q) for q in qB])
    poses = np.stack([random_pose(rng) for _ in range(2)])
    plain = env.pose_cloud(pts, geom, theta, dtype=np.float64)
    placed = env.pose_cloud(pts, geom, theta, poses=poses, dtype=np.float64)
    assert np.array_equal(plain["point_link"], tree.link_of_geoms(cm)[geom])
    worst = 0.0
    for b in range(2):
        want = geom_truth(cm, qA, qB[b], geom, pts.astype(np.float64))
        worst = max(worst, np.abs(plain["points"][b] - want).max(),
                    np.abs(placed["points"][b] - (want @ poses[b, :3, :3].T + poses[b, :3, 3])).max())
    moved = np.abs(plain["points"] - pts.astype(np.float64)).max()
    print(f"{name}: against geom_poses {worst:.3g} m (the cloud moves by up to {moved:.3g} m)")
    assert worst <= TOL
    f32 = env.pose_cloud(pts, geom, theta, poses=poses)
    assert f32["points"].dtype == np.float32
    assert np.array_equal(bits(f32["points"]), bits(placed["points"].astype(np.float32)))


def test_pose_gripper_cloud_cli(tmp_path, monkeypatch):
    from mgs.cli import pose_gripper_cloud, scan_gripper
    from mgs.cli._hydra import compose
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path))
    size = [f"width={SCAN_SIZE}", f"height={SCAN_SIZE}"]
    scan_path = scan_gripper.run(["gripper=allegro", "num_images=4", "num_points=128"] + size)
    cfg = compose("pose_gripper_cloud", ["gripper=allegro"])
    env = scan_gripper.env_at_config(cfg)
    rng = np.random.default_rng(4)
    names = env.gripper.get_actuator_joint_names()
    cm = env.model
    rngs = np.array([cm.jnt_range[cm.jnt_names.index(n)] for n in names])
    joints = rng.uniform(rngs[:, 0], rngs[:, 1], (2, len(names)))
    poses = np.stack([random_pose(rng) for _ in range(2)])
    os.makedirs(tmp_path / "grasps")
    gpath = str(tmp_path / "grasps" / "inference_grasps.npz")
    np.savez(gpath, pose=poses, joints=joints)
    out = pose_gripper_cloud.run(["gripper=allegro", f"scan={scan_path}", f"grasps={gpath}"])
    assert out == str(tmp_path / "grasps" / "gripper_clouds.npz")
    z, scan = np.load(out, allow_pickle=False), np.load(scan_path, allow_pickle=False)
    p = len(scan["points"])
    print(f"{p} points in the scan file")
    assert p > 0 and set(z.files) == {"points", "point_link", "joint_names"}
    assert z["points"].shape == (2, p, 3) and z["points"].dtype == np.float32
    assert z["point_link"].shape == (p,) and z["point_link"].dtype == np.int32
    tree = env.kinematic_tree()
    assert z["joint_names"].tolist() == tree.joint_names
    want = env.pose_cloud(scan["points"], scan["point_geom"], tree.theta_from_named(joints, names), poses=poses)
    assert np.array_equal(bits(z["points"]), bits(want["points"])) and np.array_equal(z["point_link"], want["point_link"])
    # and that cloud is the scan's geoms at the grasp's joints, placed at the grasp
    q = env.qpos.copy()
    q[env.get_joint_idxs(names)] = joints[0]
    truth = geom_truth(cm, env.qpos, q, scan["point_geom"], scan["points"].astype(np.float64))
    truth = truth @ poses[0, :3, :3].T + poses[0, :3, 3]
    assert np.abs(z["points"][0] - truth).max() <= 2.0 ** -23      # float32 rounding of coordinates below 1 m
