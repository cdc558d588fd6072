"""What the device skip of the rollouts behind the first K stable grasps
(mgs_schedule.enough_stable, the envs' WORK_SKIP) buys on a filter_to_stable
call: the headline pair (Robotiq x 003_cracker_box), the 65,536-candidate file
of the bench's large API call (8192 seeded candidates repeated 8 times, 9,384 of
them collision free), h200, K = 1000, through env.evaluate.

Three settings alternate in one process, RUNS times each after one warm-up
round: skip off (every collision-free candidate simulated, the first-K rule
applied afterwards), skip on (the envs' default: no rotation in a call that
can skip) and skip on with the rotation of YIELD_EVERY kept.  Host clock
around the synchronous calls.  Per run: ms, rollouts executed (collision free
minus skipped), skipped; and whether the returned masks are identical between
the settings.  Needs the GPU.

    python tools/filter_to_stable_rate.py [profiles/r10_enough_stable_skip.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mj-grasp-sim_amd")]
K, REPEAT, RUNS = 1000, 8, 3


def main():
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("filter_to_stable_rate: no GPU")
    torch.cuda.init()
    from mgs.env.gravityless_object_grasping import GravitylessObjectGrasping
    from mgs.gripper.robotiq2f85 import GripperRobotiq2f85
    from mgs.obj.selector import get_object
    from mgs.sampler.antipodal import robotiq_candidates
    from mgs.util.geo.transforms import SE3Pose

    class Env(GravitylessObjectGrasping):
        """counts what each rollout call ran"""

        def rollout(self, plan, **kw):
            res = super().rollout(plan, **kw)
            self.counts = (len(plan.qpos_init), int(res["skipped"]))
            return res

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_enough_stable_skip.json")
    env = Env(GripperRobotiq2f85(SE3Pose(np.zeros(3), np.array([1.0, 0, 0, 0]), "wxyz")),
              get_object("003_cracker_box"))
    H, J, _ = robotiq_candidates(env.obj, 8192, seed=0)
    poses = SE3Pose.from_mat(np.tile(np.asarray(H), (REPEAT, 1, 1)))
    J = np.tile(J, (REPEAT, 1))
    settings = [("skip off", False, 0), ("skip on", True, 0), ("skip on, rotation kept", True, env.YIELD_EVERY)]
    runs = {name: [] for name, _, _ in settings}
    masks = {}
    for it in range(RUNS + 1):
        for name, skip, ye in settings:
            env.WORK_SKIP, env.SKIP_YIELD_EVERY = skip, ye
            t = time.perf_counter()
            free, stable = env.evaluate(poses, J, horizon="h200", enough_stable=K)
            ms = (time.perf_counter() - t) * 1e3
            n, skipped = env.counts
            assert n == int(free.sum())
            masks.setdefault(name, (free, stable))
            same = bool(np.array_equal(masks[name][0], free) and np.array_equal(masks[name][1], stable))
            if it:      # round 0 warms up
                runs[name].append(dict(ms=round(ms, 2), collision_free=n, rollouts=n - skipped, skipped=skipped,
                                       stable=int(stable.sum()), same_as_first_run=same))
            print(f"round {it} {name:24s} {ms:8.1f} ms  {n - skipped:5d} rollouts, {skipped:5d} skipped, "
                  f"{int(stable.sum())} stable", flush=True)
    ref = masks["skip off"]
    identical = all(np.array_equal(m[0], ref[0]) and np.array_equal(m[1], ref[1]) for m in masks.values()) and \
        all(r["same_as_first_run"] for rs in runs.values() for r in rs)
    summary = {}
    for name, rs in runs.items():
        ms = [r["ms"] for r in rs]
        summary[name] = dict(ms_mean=round(float(np.mean(ms)), 2), ms_spread=round(max(ms) - min(ms), 2),
                             rollouts=[r["rollouts"] for r in rs], skipped=[r["skipped"] for r in rs])
    doc = dict(what="env.evaluate, Robotiq x 003_cracker_box, 8192 seeded candidates x 8, h200, enough_stable 1000",
               candidates=len(J), enough_stable=K, runs_each=RUNS, masks_identical=bool(identical), summary=summary,
               runs=runs)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(masks_identical=bool(identical), summary=summary)))
    if not identical:
        sys.exit("filter_to_stable_rate: the masks differ between the settings")


if __name__ == "__main__":
    main()
