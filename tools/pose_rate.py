"""Cost of posing a scanned gripper cloud on the MI355X (mgs_pose_cloud): the
Shadow Hand table at B joint states x P points.  One JSON line per case,
printed and written to --out (default profiles/pose_rate.jsonl):

  * the kernel time by HIP events (median of --repeat calls after a first one);
  * the bytes the call has to move -- B P 3 values out, plus the points, their
    links and the joint values in once -- over that time, and the fraction of
    the 8 TB/s HBM peak this is (the points are re-read per joint state from
    cache: they are counted once);
  * in the same run the wall time of the numpy restatement
    (tests/pose_truth.pose_kernel) on a slice of the joint states, scaled to B,
    and that the device result equals it bit for bit on the slice.

    python tools/pose_rate.py [--repeat 3] [--slice 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mj-grasp-sim_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

HBM_PEAK = 8.0e12      # bytes / s

CASES = [dict(label="grasp_batch", B=8192, P=4096, dtype="float32"),
         dict(label="one_state_dense", B=1, P=100000, dtype="float32")]


def measure(case, a):
    import pose_truth as PT
    from mgs.core.engine import pose_cloud
    from mgs.sampler.kin.model import ShadowKinematicsModel
    from mgs.sampler.kin.tree import tree_from_kinematics
    kin = ShadowKinematicsModel()
    rng = np.random.default_rng(0)
    lo, hi = kin.joint_ranges[:, 0], kin.joint_ranges[:, 1]
    tree = tree_from_kinematics(kin, theta_scan=rng.uniform(lo, hi))
    B, P, dt = case["B"], case["P"], np.dtype(case["dtype"])
    pts = rng.uniform(-0.3, 0.3, (P, 3))
    link = rng.integers(0, tree.nlink + 1, P).astype(np.int32)
    theta = rng.uniform(lo, hi, (B, tree.nlink))
    ms, res = [], None
    for _ in range(a.repeat + 1):          # the first call also starts the runtime
        res = pose_cloud(tree, pts, link, theta, dtype=dt)
        ms.append(res["kernel_ms"])
    med = float(np.median(ms[1:]))
    nbytes = B * P * 3 * dt.itemsize + P * (24 + 4) + B * tree.nlink * 8 + B * tree.nlink * 56
    ns = min(a.slice, B)
    t0 = time.perf_counter()
    want, wlinks = PT.pose_kernel(tree, pts, link, theta[:ns])
    t_host = time.perf_counter() - t0
    same = bool(np.array_equal(res["points"][:ns].view(np.int32), want.astype(dt).view(np.int32)) and
                np.array_equal(res["links"][:ns].view(np.int64), wlinks.view(np.int64)))
    line = {"case": case["label"], "B": B, "P": P, "nlink": tree.nlink, "dtype": dt.name,
            "kernel_ms": round(med, 4), "kernel_ms_runs": [round(v, 4) for v in ms[1:]],
            "first_call_kernel_ms": round(ms[0], 4), "bytes": int(nbytes),
            "bytes_per_s": round(nbytes / (med * 1e-3), 1), "fraction_of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 4),
            "numpy_slice_states": ns, "numpy_slice_s": round(t_host, 4), "numpy_scaled_s": round(t_host * B / ns, 2),
            "numpy_over_kernel": round(t_host * B / ns * 1e3 / med, 1), "slice_bit_exact": same}
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--slice", type=int, default=2, help="joint states the numpy truth poses")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_rate.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()          # one line per case of this run
    for case in CASES:
        measure(case, a)


if __name__ == "__main__":
    main()
