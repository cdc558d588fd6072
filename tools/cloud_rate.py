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

--batch S1,S2,...: many scenes per call instead.  S copies of the pile, each
turned about the world z by another angle (distinct clouds, the same work);
per S one JSON line appended to --out: the wall time of S mgs_scan_cloud calls
one after the other, that of one mgs_scan_cloud_batch call with its per-scene
stages and the shared pick, their ratio, pick_ms / S, and the device memory in
use before the batched call and at its largest (hipMemGetInfo, sampled by a
thread every few milliseconds while the call runs).  Medians of --repeat runs
after a first one, each with its runs.  --single-only: the sequential calls
alone (a library without the batch entries: MGS_LIB_MAIN names it).
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


def turned(arrays, angle):
    """the scene's arrays with every drawable turned about the world z"""
    c, s = np.cos(angle), np.sin(angle)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    out = dict(arrays)
    out["draw_pos"] = np.ascontiguousarray(arrays["draw_pos"] @ Rz.T)
    out["draw_rot"] = np.ascontiguousarray(Rz @ arrays["draw_rot"])
    return out


def mem_used():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def with_peak(fn):
    """(fn(), device bytes in use before it, the most seen while it ran)"""
    import threading
    before = mem_used()
    peak, done = [before], threading.Event()

    def sample():
        while not done.wait(0.003):
            peak[0] = max(peak[0], mem_used())
    th = threading.Thread(target=sample)
    th.start()
    try:
        out = fn()
    finally:
        done.set()
        th.join()
    return out, before, peak[0]


def measure_batch(env, S, a):
    from mgs.core import engine
    from mgs.scan.scene import REGION
    extr, K, Kp = env._cloud_cameras(a.views, a.size, a.size)
    base = env.scan_scene().arrays()
    scenes = [turned(base, 2 * np.pi * j / S) for j in range(S)]
    col = env.scan_colors()
    cams = (extr[:, :3, 3], extr[:, :3, :3], a.size, a.size, K[0, 0], K[1, 1], K[0, 2], K[1, 2], extr, Kp[0, 0], Kp[1, 1],
            Kp[0, 2], Kp[1, 2])
    kw = dict(voxel_size=0.002, erode_iters=5, region=REGION, device=env.device)

    def sequential():
        return [engine.scan_cloud(sc, *cams, col, a.points, **kw) for sc in scenes]

    def batched():
        return engine.scan_cloud_batch(scenes, [col] * S, a.points, *cams, **kw)
    seq_runs, bat_runs, stage_runs, peaks = [], [], [], []
    seq = bat = None
    for _ in range(a.repeat + 1):          # the first call also starts the runtime
        seq, t = wall(sequential)
        seq_runs.append(t)
        if not a.single_only:
            (bat, t), before, peak = with_peak(lambda: wall(batched))
            bat_runs.append(t)
            peaks.append((before, peak))
            stage_runs.append([float(np.sum([r[2][k] for r in bat])) for k in ("render_ms", "points_compact_ms", "voxels_ms")]
                              + [bat[0][2]["pick_ms"]])
    line = {"case": "batch", "scenes": S, "views": a.views, "width": a.size, "height": a.size, "num_points": a.points,
            "library": os.environ.get("MGS_LIB_MAIN", "libmgs_gpu.so"),
            "voxels": [r[2]["voxels"] for r in seq][:4], "single_pick_ms": [round(r[2]["pick_ms"], 3) for r in seq][:4],
            "sequential_s": round(float(np.median(seq_runs[1:])), 4), "sequential_s_runs": [round(t, 4) for t in seq_runs[1:]]}
    if not a.single_only:
        med = np.median(np.array(stage_runs[1:]), axis=0)
        line.update({
            "batch_s": round(float(np.median(bat_runs[1:])), 4), "batch_s_runs": [round(t, 4) for t in bat_runs[1:]],
            "sequential_over_batch": round(float(np.median(seq_runs[1:]) / np.median(bat_runs[1:])), 2),
            "batch_render_ms_sum": round(med[0], 3), "batch_points_compact_ms_sum": round(med[1], 3),
            "batch_voxels_ms_sum": round(med[2], 3), "batch_pick_ms": round(med[3], 3),
            "batch_pick_ms_runs": [round(r[3], 3) for r in stage_runs[1:]],
            "batch_pick_ms_per_scene": round(med[3] / S, 3),
            "batch_pick_us_per_pick": round(med[3] * 1e3 / max(1, a.points), 3),
            "device_mib_before": round(peaks[-1][0] / 2 ** 20, 1), "device_mib_peak": round(max(p for _, p in peaks) / 2 ** 20, 1),
            "equal_bit_for_bit": bool(all(np.array_equal(s[0].view(np.int32), b[0].view(np.int32))
                                          and np.array_equal(s[1].view(np.int32), b[1].view(np.int32))
                                          for s, b in zip(seq, bat))),
            "distinct_clouds": len({s[0].tobytes() for s in seq})})
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
    ap.add_argument("--batch", default=None, help="scene counts, e.g. 1,16,64,256: the many-scenes mode")
    ap.add_argument("--single-only", action="store_true", help="with --batch: the sequential single-scene calls alone")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    env = pile_env()
    if a.batch:
        for S in (int(v) for v in a.batch.split(",")):
            measure_batch(env, S, a)
        return
    open(a.out, "w").close()          # one line per case of this run
    measure(env, "shipped_meshes", a)
    from scan_truth import icosphere
    ball = icosphere(4, radius=0.04)
    env._scan_meshes = {os.path.join(o.asset_dir, o.info()["original_file"]): ball for o in env.objects}
    measure(env, "sphere_5120_faces", a)


if __name__ == "__main__":
    main()
