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
(mgs_scan_cloud; same file layout, DESIGN 5b for how the two clouds differ).

`ids=<a>:<b>` (half-open; `ids=all`: every scene directory) with `cloud=device`
writes the scene_pcd.npz of many scenes, `batch` of them per call of
mgs.env.clutter_table.scan_clouds (their farthest-point picks in one launch);
each file is what `id=<k> cloud=device` writes.  Under a launched world every
rank takes its contiguous share of the list (mgs.env.sharding.shard_bounds)."""
import os
import sys

import numpy as np

from mgs.cli._hydra import compose
from mgs.env.selector import get_env_from_dict, load_scene
from mgs.env.sharding import cli_device, launch_world, shard_bounds
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


def parse_ids(spec, nscene=None):
    """the scene numbers of the key `ids`: "<a>:<b>" is a, ..., b - 1; "all"
    every scene directory (needs nscene).  With nscene, numbers past the last
    directory are refused."""
    spec = str(spec).strip()
    if spec == "all":
        if nscene is None:
            raise ValueError("ids=all needs the scene directories")
        return list(range(nscene))
    parts = spec.split(":")
    try:
        a, b = (int(q) for q in parts)
    except ValueError:
        raise ValueError(f"ids={spec!r}: <first>:<past the last> or all") from None
    if a < 0 or b < a:
        raise ValueError(f"ids={spec!r}: need 0 <= first <= past the last")
    if nscene is not None and b > nscene:
        raise ValueError(f"ids={spec!r}: there are {nscene} scene directories")
    return list(range(a, b))


def rank_ids(ids, world, rank):
    """this rank's contiguous share of the list"""
    lo, hi = shard_bounds(len(ids), world, rank)
    return list(ids[lo:hi])


def split_args(args):
    """(the value of ids= or None, whether id= is given, the other overrides):
    `ids` is taken out before the values are read as YAML, which would read
    2:5 as a base-60 number"""
    ids, rest = None, []
    for a in args:
        key = a.split("=", 1)[0].lstrip("+")
        if key == "ids" and "=" in a:
            ids = a.split("=", 1)[1]
        else:
            rest.append(a)
    return ids, any(a.split("=", 1)[0].lstrip("+") == "id" for a in rest), rest


def check_keys(cfg, id_given):
    """an unknown `cloud`, `ids` without cloud=device, `ids` beside `id`: a
    ValueError before anything is read or scanned"""
    path = cloud_path(cfg)
    if cfg.get("ids") is None:
        return
    if path != "device":
        raise ValueError("ids= writes many scenes through the batched device path: it needs cloud=device")
    if id_given:
        raise ValueError("ids= and id= name the scenes twice: give one of them")
    if str(cfg.ids).strip() != "all":
        parse_ids(cfg.ids)
    if int(cfg.get("batch", 64)) < 1:
        raise ValueError("batch must be at least 1")


def write_cloud(output_dir, cfg, scene, points, colors):
    out = os.path.join(output_dir, cfg.gripper.name, scene)
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "scene_pcd"), points=points, colors=colors)


def many_clouds(cfg, root, scenes, output_dir, voxel_size=0.002):
    """scene_pcd.npz of this rank's share of cfg.ids, cfg.batch scenes per call"""
    from mgs.env.clutter_table import scan_clouds
    rank, world = launch_world()
    ids = rank_ids(parse_ids(cfg.ids, len(scenes)), world, rank)
    batch, num_points = int(cfg.get("batch", 64)), int(cfg.get("num_points", 15000))
    for lo in range(0, len(ids), batch):
        names = [scenes[k] for k in ids[lo:lo + batch]]
        envs = [get_env_from_dict(cfg.env, load_scene(os.path.join(root, name, "scene.npz")), device=cli_device())
                for name in names]
        clouds = scan_clouds(envs, int(cfg.num_images), num_points=num_points, voxel_size=voxel_size,
                             width=int(cfg.get("width", 480)), height=int(cfg.get("height", 480)), batch=batch)
        for name, (points, colors) in zip(names, clouds):
            print("Scene dir: ", os.path.join(root, name))
            if len(points) < num_points:
                print(f"only {len(points)} points after downsampling (num_points={num_points}): all kept")
            write_cloud(output_dir, cfg, name, points, colors)


def run(argv=None):
    ids, id_given, args = split_args(sys.argv[1:] if argv is None else list(argv))
    cfg = compose("render_scene_proc", args)
    if ids is not None:
        cfg["ids"] = ids
    check_keys(cfg, id_given)      # a bad key stops here, before anything is read or scanned
    output_dir = os.getenv("MGS_OUTPUT_DIR")
    input_dir = os.getenv("MGS_INPUT_DIR")
    assert output_dir is not None, "No output_dir defined!"
    assert input_dir is not None, "No input_dir defined!"
    root = os.path.join(input_dir, cfg.gripper.name)
    scenes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    if cfg.get("ids") is not None:
        many_clouds(cfg, root, scenes, output_dir)
    else:
        scene = scenes[int(cfg.id)]
        print("Scene dir: ", os.path.join(root, scene))
        points, colors = scene_cloud(cfg, load_scene(os.path.join(root, scene, "scene.npz")))
        write_cloud(output_dir, cfg, scene, points, colors)
    print("Finished!")


if __name__ == "__main__":
    run()
