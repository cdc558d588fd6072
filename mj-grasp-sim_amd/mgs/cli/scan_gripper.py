"""python -m mgs.cli.scan_gripper gripper=<cfg> [qpos=[...]] [file_id=open]
(reference: mgs/cli/scan_gripper.py:29-81).

Scan the gripper itself at a joint state from `num_images` Fibonacci views on
the GPU (GripperScanEnv: the collision geometry, depth and geom segmentation by
ray casting, flat grey) and write $MGS_OUTPUT_DIR/<file_id>_<hash>.npz (`.` if
the variable is unset), the gripper representation a multi-embodiment grasp
network is conditioned on.  The file needs no pickle:

  scans (N, H, W, 4) float32, scan_extrinsics (N, 4, 4), scan_intrinsics (3, 3),
  scan_masks (N, H, W) bool                                  as the reference
  segment_names (nseg,) str, segments (nseg, N, H, W) bool   for its pickled dict
  geom_names (ngeom,) str, segmentation (N, H, W) int32
  points (P, 3) float32, point_geom (P,) int32, point_segments (nseg, P) bool

Segments are the geoms each joint moves (one per hinge or slide joint, then
`body`), or the `gripper.segmentation` mapping segment name -> joint name.
"""
import os

import numpy as np

from mgs.cli._hydra import main
from mgs.env.gripper_scan import GripperScanEnv
from mgs.env.sharding import cli_device
from mgs.gripper.selector import get_gripper
from mgs.obj.selector import generate_unique_hash


def env_at_config(cfg):
    """the scan env at the joint state the configuration names"""
    gripper = get_gripper(cfg.gripper)
    env = GripperScanEnv(gripper, device=cli_device())
    state = cfg.gripper.get("state")
    if state is not None:
        env.set_state(np.array(state, dtype=np.float64))
    else:
        qpos = cfg.get("qpos")
        if qpos is None or isinstance(qpos, str):       # absent, or an interpolation left unresolved
            qpos = cfg.gripper.qpos
        env.set_qpos(np.array(qpos, dtype=np.float64), env.get_joint_idxs(gripper.get_actuator_joint_names()))
    return env


def scan(cfg):
    """the env after its scan, and what the scan returned"""
    env = env_at_config(cfg)
    images, extrinsics, image_masks, segmentation = env.scan(
        num_images=int(cfg.num_images), width=int(cfg.get("width", 480)), height=int(cfg.get("height", 480)))
    return env, images, extrinsics, image_masks, segmentation


@main("scan_gripper")
def run(cfg):
    output_dir = os.getenv("MGS_OUTPUT_DIR") or "."
    env, images, extrinsics, image_masks, segmentation = scan(cfg)
    spec = cfg.gripper.get("segmentation")
    spec = None if spec is None else dict(spec)
    names, segments = env.segments(segmentation, image_masks, spec)
    points, point_geom, point_segments = env.cloud(int(cfg.get("num_points", 4096)), spec=spec)
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f"{cfg.file_id}_{generate_unique_hash()}.npz")
    np.savez(path, scans=images, scan_extrinsics=extrinsics, scan_intrinsics=env.get_camera_intrinsics(),
             scan_masks=image_masks, segment_names=np.array(names, dtype=np.str_), segments=segments,
             geom_names=np.array(env.scan_geom_names, dtype=np.str_), segmentation=segmentation, points=points,
             point_geom=point_geom, point_segments=point_segments)
    print("Finished!", path)
    return path


if __name__ == "__main__":
    run()
