"""python -m mgs.cli.pose_gripper_cloud gripper=<cfg> scan=<scan_gripper npz> grasps=<npz with pose, joints>

The scanned gripper cloud at every grasp of a file: what the reference's
kinematic_pcd_transform (mgs/sampler/kin/base.py:34-77) gives the
multi-embodiment network for each grasp it scores, on the GPU
(GripperScanEnv.pose_cloud, mgs_pose_cloud).

The gripper configuration (and `qpos=`, as for scan_gripper) names the joint
state the scan was taken at; the kinematic tree is rebuilt from it.  A point's
link comes from the scan file's `point_geom`; the grasps' `joints` are the
values of the gripper's actuated joints (get_actuator_joint_names order), every
other joint stays at its rest position; `pose` (B, 4, 4), contact frame, places
each cloud in the scene (place=false leaves it in the scan's frame).  Written
next to the grasps, gripper_clouds.npz:

  points (B, P, 3) float32, point_link (P,) int32 (0 = base, k = link k - 1),
  joint_names (nlink,) str
"""
import os

import numpy as np

from mgs.cli._hydra import main
from mgs.cli.scan_gripper import env_at_config


def joint_values_to_theta(env, tree, joints):
    """theta (B, nlink) of the grasps' actuated-joint values"""
    names = env.gripper.get_actuator_joint_names()
    joints = np.asarray(joints, np.float64)
    if joints.ndim != 2 or joints.shape[1] != len(names):
        raise ValueError(f"joints is (B, {len(names)}) for this gripper, not {joints.shape}")
    if all(n in tree.joint_names for n in names):
        return tree.theta_from_named(joints, names)
    # a list that names a joint the model lacks (the Robotiq's): resolved as the
    # scan resolves it, by GripperScanEnv.set_qpos on the model's addresses
    q = np.tile(env.model.qpos0, (len(joints), 1))
    for k, a in enumerate(env.get_joint_idxs(names)):
        q[:, int(a)] = joints[:, k]
    return tree.theta_from_qpos(q)


@main("pose_gripper_cloud")
def run(cfg):
    if not cfg.get("scan") or not cfg.get("grasps"):
        raise ValueError("pose_gripper_cloud needs scan=<scan_gripper npz> and grasps=<npz with pose, joints>")
    env = env_at_config(cfg)
    scan = np.load(str(cfg.scan))
    grasps = np.load(str(cfg.grasps))
    points, point_geom = scan["points"], scan["point_geom"]
    if list(scan["geom_names"]) != env.scan_geom_names:
        raise ValueError(f"{cfg.scan} is a scan of another gripper model than gripper={cfg.gripper.get('name')}")
    tree = env.kinematic_tree()
    theta = joint_values_to_theta(env, tree, grasps["joints"])
    poses = np.asarray(grasps["pose"], np.float64) if cfg.get("place", True) else None
    res = env.pose_cloud(points, point_geom, theta, poses=poses, dtype=np.float32)
    path = os.path.join(os.path.dirname(os.path.abspath(str(cfg.grasps))), "gripper_clouds.npz")
    np.savez(path, points=res["points"], point_link=res["point_link"],
             joint_names=np.array(tree.joint_names, dtype=np.str_))
    print(f"Finished! {path}: {res['points'].shape[0]} clouds of {res['points'].shape[1]} points, "
          f"kernel {res['kernel_ms']:.3f} ms")
    return path


if __name__ == "__main__":
    run()
