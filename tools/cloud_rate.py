"""Cost of the scene cloud on the MI355X: 32 views of 480 x 480 of the golden
pile scene (tests/golden/clutter_scene.npz) down to 15 000 points, in the two
mesh cases of tools/scan_rate.py.  One JSON line per case, printed and written
to --out (default profiles/cloud_rate.jsonl):

  * the device stages of mgs_scan_cloud (HIP events, median of --repeat calls
    after a first one): render, points + compaction, voxels, pick;
  * in the same run the wall time of the host functions the middle stages
    replace: rgbd_to_pcd + mask + crop, voxel_downsample_pcd;
  * mgs_contact_fps and mgs_scan_fps on the same float32-rounded voxel cloud
    (device time and wall time of each), whether their indices agree, and the
    pick's distance evaluations over the sweep's n (k - 1);
  * wall time of the CLI's scene_cloud with cloud=host and cloud=device, and
    how many rows of the two clouds differ.

    python tools/cloud_rate.py [--views 32] [--size 480] [--points 15000] [--repeat 3]
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

from scan_rate import pile_env  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def rows_differing(a, b):
    """(rows of a not among the rows of b, rows that differ place by place or
    None when the lengths differ)"""
    key = lambda x: {r.tobytes() for r in np.ascontiguousarray(x)}      # noqa: E731
    missing = len(key(a) - key(b))
    same_len = len(a) == len(b)
    return missing, (int(np.any(a.view(np.int32) != b.view(np.int32), axis=1).sum()) if same_len else None)


def measure(env, label, a):
    from mgs.cli import render_scene_processed as R
    from mgs.cli._hydra import compose
    from mgs.core.engine import contact_fps, scan_fps
    from mgs.scan.scene import REGION
    from mgs.util.img_proc import rgbd_to_pcd, voxel_downsample_pcd
    stages = []
    for _ in range(a.repeat + 1):          # the first call also starts the runtime
        env.scan_cloud(a.views, num_points=a.points, width=a.size, height=a.size)
        stages.append(dict(env.last_cloud))
    info = stages[-1]
    med = {k: float(np.median([s[k] for s in stages[1:]])) for k in ("render_ms", "points_compact_ms", "voxels_ms", "pick_ms")}
    # the host functions of the same views
    rgbd, extr, masks, seg = env.scan(num_images=a.views, width=a.size, height=a.size)
    K = env.get_camera_intrinsics()

    def crop():
        pcd, feat = rgbd_to_pcd(rgbd, K, extr)
        pcd, feat = pcd[masks], feat[masks]
        inside = np.all((pcd < REGION[None, 3:]) & (pcd > REGION[None, :3]), axis=-1)
        return pcd[inside], feat[inside]
    (pcd, feat), t_pcd = wall(crop)
    (vox, _), t_vox = wall(lambda: voxel_downsample_pcd(pcd, feat, 0.002))
    # the two picks on one cloud
    x = vox.astype(np.float32)
    k = min(a.points, len(x))
    (brute, brute_ms), t_brute = wall(lambda: contact_fps(x, k, device=env.device))
    (pruned, nevals, pruned_ms), t_pruned = wall(lambda: scan_fps(x, k, 8 * 0.002, device=env.device))
    # the CLI function both ways, on this env
    R.get_env_from_dict = lambda cfg, scene_def, **kw: env
    base = ["gripper=robotiq_2f_85", f"num_images={a.views}", f"width={a.size}", f"height={a.size}",
            f"num_points={a.points}"]
    (hp, hc), t_host = wall(lambda: R.scene_cloud(compose("render_scene_proc", base + ["cloud=host"]), None))
    (dp, dc), t_dev = wall(lambda: R.scene_cloud(compose("render_scene_proc", base + ["cloud=device"]), None))
    missing, placewise = rows_differing(dp, hp)
    dev_mid = med["points_compact_ms"] + med["voxels_ms"]
    line = {
        "case": label, "views": a.views, "width": a.size, "height": a.size, "num_points": a.points,
        "kept_device": info["kept"], "kept_host": int(len(pcd)), "voxels_device": info["voxels"],
        "voxels_host": int(len(vox)), "grid_cells": info["grid_cells"],
        **{k: round(v, 3) for k, v in med.items()},
        "stage_ms_runs": [[round(s[k], 3) for k in ("render_ms", "points_compact_ms", "voxels_ms", "pick_ms")] for s in stages[1:]],
        "host_rgbd_to_pcd_crop_s": round(t_pcd, 4), "host_voxel_downsample_s": round(t_vox, 4),
        "host_over_device_points_to_voxels": round((t_pcd + t_vox) * 1e3 / dev_mid, 1),
        "fps_n": int(len(x)), "fps_k": int(k), "contact_fps_ms": round(brute_ms, 3), "scan_fps_ms": round(pruned_ms, 3),
        "contact_fps_wall_s": round(t_brute, 4), "scan_fps_wall_s": round(t_pruned, 4),
        "fps_indices_equal": bool(np.array_equal(brute, pruned)),
        "pick_evals": int(nevals), "pick_evals_fraction": round(nevals / max(1, len(x) * (k - 1)), 5),
        "cloud_pick_evals": info["pick_evals"],
        "scene_cloud_host_s": round(t_host, 4), "scene_cloud_device_s": round(t_dev, 4),
        "rows_host": int(len(hp)), "rows_device": int(len(dp)), "device_rows_not_in_host": missing,
        "rows_differing_in_place": placewise,
        "colors_equal_in_place": bool(len(hc) == len(dc) and np.array_equal(hc, dc)),
    }
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--points", type=int, default=15000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_rate.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()          # one line per case of this run
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    env = pile_env()
    measure(env, "shipped_meshes", a)
    from scan_truth import icosphere
    ball = icosphere(4, radius=0.04)
    env._scan_meshes = {os.path.join(o.asset_dir, o.info()["original_file"]): ball for o in env.objects}
    measure(env, "sphere_5120_faces", a)


if __name__ == "__main__":
    main()
