"""Rate of the scene scan on the MI355X: 32 views of 480 x 480 of the golden
pile scene (tests/golden/clutter_scene.npz), once with the shipped visual
meshes and once with every object's mesh replaced by a 5120-face sphere (an
icosahedron subdivided 4 times, the size class of a deep tree).  Prints one
JSON line per case: rays/s and kernel_ms of mgs_scan_render, the mean
ray-triangle tests per ray, kernel_ms of mgs_scan_points, and the host costs
around them (scene + BVH build, rgbd_to_pcd, voxel_downsample_pcd at 2 mm).
A last line is the gripper scan: the Shadow hand's collision geometry
(capsules, cylinders, boxes, spheres, hulls) from 10 views of 480 x 480
(GripperScanEnv.scan).

    python tools/scan_rate.py [--views 32] [--size 480] [--repeat 3] [--gripper-views 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mj-grasp-sim_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def pile_env():
    from make_clutter_scene import make_env
    from mgs.env.clutter_table import ClutterTableEnv
    env = make_env()
    z = np.load(os.path.join(ROOT, "tests", "golden", "clutter_scene.npz"))
    return ClutterTableEnv.from_dict({"gripper": env.gripper, "objects": env.objects,
                                      "env_state": {"state": z["state"]}})


def measure(env, label, views, size, repeat):
    from mgs.core.engine import scan_points
    from mgs.scan.scene import REGION
    from mgs.util.img_proc import rgbd_to_pcd, voxel_downsample_pcd
    t0 = time.perf_counter()
    scene = env.scan_scene()
    scene.arrays()
    t_scene = time.perf_counter() - t0
    ms = []
    for _ in range(repeat + 1):          # the first call also starts the runtime
        rgbd, extr, masks, seg = env.scan(num_images=views, width=size, height=size)
        ms.append(env.last_scan["kernel_ms"])
    ms = ms[1:]
    res = env.last_scan
    K = env.get_camera_intrinsics()
    _, keep, ms_points = scan_points(res["depth"], seg, extr, K[0, 0], K[1, 1], K[0, 2], K[1, 2], device=env.device)
    t0 = time.perf_counter()
    pcd, feat = rgbd_to_pcd(rgbd, K, extr)
    pcd, feat = pcd[masks], feat[masks]
    inside = np.all((pcd < REGION[None, 3:]) & (pcd > REGION[None, :3]), axis=-1)
    pcd, feat = pcd[inside], feat[inside]
    t_pcd = time.perf_counter() - t0
    t0 = time.perf_counter()
    vox, _ = voxel_downsample_pcd(pcd, feat, 0.002)
    t_vox = time.perf_counter() - t0
    rays = views * size * size
    print(json.dumps({
        "case": label, "views": views, "width": size, "height": size, "triangles": int(sum(m.ntri for m in scene.meshes)),
        "instances": int(scene.ndraw - 2), "kernel_ms": round(float(np.median(ms)), 3),
        "kernel_ms_runs": [round(float(x), 3) for x in ms], "rays_per_s": round(rays / (np.median(ms) * 1e-3)),
        "mean_ntest_per_ray": round(float(res["ntest"].mean()), 3), "hit_fraction": round(float((seg != -1).mean()), 4),
        "points_kernel_ms": round(ms_points, 3), "points_kept_device": int(keep.sum()), "points_kept_host": int(len(pcd)),
        "host_scene_build_s": round(t_scene, 3), "host_rgbd_to_pcd_crop_s": round(t_pcd, 3),
        "host_voxel_downsample_s": round(t_vox, 3), "voxels": int(len(vox))}), flush=True)


def measure_gripper(views, size, repeat):
    """GripperScanEnv.scan of the open Shadow hand: kernel time by HIP events,
    median of `repeat` after a first call"""
    from mgs.env.gripper_scan import GripperScanEnv
    from mgs.gripper.shadow import GripperShadowRight
    from mgs.util.geo.transforms import SE3Pose
    env = GripperScanEnv(GripperShadowRight(SE3Pose(np.zeros(3), np.array([1.0, 0, 0, 0]), "wxyz")))
    t0 = time.perf_counter()
    scene = env.scan_scene()
    S = scene.arrays()
    t_scene = time.perf_counter() - t0
    ms = []
    for _ in range(repeat + 1):
        _, _, masks, seg = env.scan(num_images=views, width=size, height=size)
        ms.append(env.last_scan["kernel_ms"])
    ms = ms[1:]
    rays = views * size * size
    kinds = np.bincount(S["draw_type"], minlength=5)
    print(json.dumps({
        "case": "gripper_shadow", "views": views, "width": size, "height": size, "drawables": int(scene.ndraw),
        "boxes": int(kinds[0]), "spheres": int(kinds[1]), "hulls": int(kinds[2]), "capsules": int(kinds[3]),
        "cylinders": int(kinds[4]), "triangles": int(sum(m.ntri for m in scene.meshes)),
        "kernel_ms": round(float(np.median(ms)), 3), "kernel_ms_runs": [round(float(x), 3) for x in ms],
        "rays_per_s": round(rays / (np.median(ms) * 1e-3)),
        "mean_ntest_per_ray": round(float(env.last_scan["ntest"].mean()), 3),
        "hit_fraction": round(float((seg != -1).mean()), 4), "masked_fraction": round(float(masks.mean()), 4),
        "host_scene_build_s": round(t_scene, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--gripper-views", type=int, default=10)
    a = ap.parse_args()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    env = pile_env()
    measure(env, "shipped_meshes", a.views, a.size, a.repeat)
    # every object's visual mesh replaced by one 5120-face sphere of the object's size class
    from scan_truth import icosphere
    ball = icosphere(4, radius=0.04)
    env._scan_meshes = {os.path.join(o.asset_dir, o.info()["original_file"]): ball for o in env.objects}
    measure(env, "sphere_5120_faces", a.views, a.size, a.repeat)
    if a.gripper_views > 0:      # 0: the pile rows alone (a library from before the gripper scan)
        measure_gripper(a.gripper_views, a.size, a.repeat)


if __name__ == "__main__":
    main()
