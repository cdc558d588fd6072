"""python -m mgs.cli.render_scene_processed gripper=<cfg> id=<k>
(reference: mgs/cli/render_scene_processed.py:16-73).

For scene directory number `id` (sorted) under $MGS_INPUT_DIR/<gripper>/: load
scene.npz, scan `num_images` views of the pile on the GPU (ClutterTableEnv.scan:
depth and geom segmentation by ray casting, flat colours), turn them into
points with the reference's intrinsics (rgbd_to_pcd), keep the eroded image
mask and the region box, voxel-downsample at 2 mm, pick `num_points` by
farthest-point sampling of the float32-rounded points (mgs_contact_fps) and
write $MGS_OUTPUT_DIR/<gripper>/<scene>/scene_pcd.npz with float32 `points`
and `colors` -- the cloud the grasp network consumes.  `cloud=device` runs
everything between the scene and the sampled rows on the GPU instead
(mgs_scan_cloud; same file layout, DESIGN 5b for how the two clouds differ)."""
import os

import numpy as np

from mgs.cli._hydra import main
from mgs.env.selector import get_env_from_dict, load_scene
from mgs.env.sharding import cli_device
from mgs.scan.scene import REGION
from mgs.util.img_proc import rgbd_to_pcd, voxel_downsample_pcd


def scan(cfg, scene_def):
    env = get_env_from_dict(cfg.env, scene_def, device=cli_device())
    images, extrinsics, image_masks, _ = env.scan(num_images=int(cfg.num_images), width=int(cfg.get("width", 480)),
                                                  height=int(cfg.get("height", 480)))
    return images, extrinsics, env.get_camera_intrinsics(), image_masks


CLOUD_PATHS = ("host", "device")


def cloud_path(cfg):
    """config key `cloud`: host (default: numpy between the images and the
    pick) or device (ClutterTableEnv.scan_cloud: everything on the GPU)"""
    path = cfg.get("cloud", "host")
    if path not in CLOUD_PATHS:
        raise ValueError(f"cloud={path!r}: one of {', '.join(CLOUD_PATHS)}")
    return path


def device_cloud(cfg, scene_def, voxel_size=0.002):
    """scene_cloud through mgs_scan_cloud: only the sampled rows leave the GPU"""
    env = get_env_from_dict(cfg.env, scene_def, device=cli_device())
    num_points = int(cfg.get("num_points", 15000))
    points, colors = env.scan_cloud(int(cfg.num_images), num_points=num_points, voxel_size=voxel_size,
                                    width=int(cfg.get("width", 480)), height=int(cfg.get("height", 480)))
    if len(points) < num_points:
        print(f"only {len(points)} points after downsampling (num_points={num_points}): all kept")
    return points, colors


def scene_cloud(cfg, scene_def, voxel_size=0.002):
    """(points, colors) float32 of one scene, at most cfg.num_points of them"""
    if cloud_path(cfg) == "device":
        return device_cloud(cfg, scene_def, voxel_size)
    from mgs.core.engine import contact_fps
    images, extrinsics, intrinsics, image_masks = scan(cfg, scene_def)
    pcd, feature = rgbd_to_pcd(images, intrinsics, extrinsics)
    pcd, feature = pcd[image_masks], feature[image_masks]
    region = np.all((pcd < REGION[None, 3:]) & (pcd > REGION[None, :3]), axis=-1)
    pcd, feature = pcd[region], feature[region]
    pcd, feature = voxel_downsample_pcd(pcd, feature, voxel_size=voxel_size)
    num_points = int(cfg.get("num_points", 15000))
    if len(pcd) >= num_points:
        idx, _ = contact_fps(pcd.astype(np.float32), num_points, device=cli_device())
        pcd, feature = pcd[idx], feature[idx]
    else:
        print(f"only {len(pcd)} points after downsampling (num_points={num_points}): all kept")
    return np.asarray(pcd, dtype=np.float32), np.asarray(feature, dtype=np.float32)


@main("render_scene_proc")
def run(cfg):
    cloud_path(cfg)      # an unknown value stops here, before anything is read or scanned
    output_dir = os.getenv("MGS_OUTPUT_DIR")
    input_dir = os.getenv("MGS_INPUT_DIR")
    assert output_dir is not None, "No output_dir defined!"
    assert input_dir is not None, "No input_dir defined!"
    root = os.path.join(input_dir, cfg.gripper.name)
    scene = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))[int(cfg.id)]
    print("Scene dir: ", os.path.join(root, scene))
    points, colors = scene_cloud(cfg, load_scene(os.path.join(root, scene, "scene.npz")))
    out = os.path.join(output_dir, cfg.gripper.name, scene)
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "scene_pcd"), points=points, colors=colors)
    print("Finished!")


if __name__ == "__main__":
    run()
