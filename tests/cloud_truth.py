"""Plain-numpy restatement of the scene-cloud stages (csrc/mgs_cloud.hip), the
truth the cloud tests compare against.  Test infrastructure only.

Every stage is written in the kernels' order of operations, so results can be
compared bit for bit; none of them calls the function it is compared with
(np.floor_divide, voxel_downsample_pcd, np.add.at).

  cells         numpy's float floor_divide by the fmod rule, for a >= 0, b > 0
  voxels        the voxel grid: cells, ascending (x, y, z) order, sums in
                ascending point index, means
  brute_fps     the sweep of mgs_contact_fps
  bucket_fps    the pruned pick of mgs_scan_fps with its evaluation count
  cloud         render -> points -> voxels -> pick (tests/scan_truth.py in front)
"""
import numpy as np

import scan_truth as T

FPS_MAX_CELLS = 1 << 24


def cells(a, b):
    """floor_divide(a, b) as int64: mod = fmod(a, b), div = (a - mod) / b, 0
    where div == 0, else floor(div), plus 1 where div - floor(div) > 0.5"""
    a = np.asarray(a, np.float64)
    mod = np.fmod(a, b)
    div = (a - mod) / b
    f = np.floor(div)
    f = np.where(div - f > 0.5, f + 1.0, f)
    return np.where(div == 0.0, 0.0, f).astype(np.int64)


def voxels(points, features, voxel_size, keep=None):
    """(positions (nvox, 3) f64, features (nvox, nfeat) float32, counts): one
    lane per voxel adds its points one after the other in ascending index, the
    positions in f64 from +0.0, the features in float32 from +0.0"""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    F = np.asarray(features, np.float32).reshape(len(P), -1)
    if keep is not None:
        P, F = P[keep], F[keep]
    nfeat = F.shape[1]
    if len(P) == 0:
        return np.zeros((0, 3)), np.zeros((0, nfeat), np.float32), np.zeros(0, np.int32)
    c = cells(P - P.min(axis=0), voxel_size)
    order = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))          # stable: ascending index inside a cell
    cs = c[order]
    first = np.concatenate([[True], np.any(cs[1:] != cs[:-1], axis=1)])
    start = np.nonzero(first)[0]
    count = np.diff(np.concatenate([start, [len(P)]]))
    psum = np.zeros((len(start), 3))
    fsum = np.zeros((len(start), nfeat), np.float32)
    for q in range(int(count.max())):
        sel = np.nonzero(count > q)[0]
        j = order[start[sel] + q]
        psum[sel] = psum[sel] + P[j]
        fsum[sel] = fsum[sel] + F[j]
    cnt = count.astype(np.float64)[:, None]
    return psum / cnt, (fsum.astype(np.float64) / cnt).astype(np.float32), count.astype(np.int32)


def _dist(x, p):
    d = x - p
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def brute_fps(x, k):
    """mgs_contact_fps: out[0] = 0; running minimum updated on d < c; next =
    the first maximum"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    out = np.zeros(k, np.int32)
    c = np.full(len(x), np.inf)
    for i in range(1, k):
        d = _dist(x, x[out[i - 1]])
        c = np.where(d < c, d, c)
        out[i] = int(np.argmax(c))
    return out


def bucket_grid(x, bucket_size, max_cells=FPS_MAX_CELLS):
    """(side, dims, flat cell per point): the side doubles until the grid over
    the bounding box has at most max_cells cells"""
    lo = x.min(axis=0)
    ext = x.max(axis=0) - lo
    side = float(bucket_size)
    while True:
        dims = np.floor(ext / side) + 1.0
        if dims[0] * dims[1] * dims[2] <= max_cells:
            break
        side = side * 2.0
    dims = dims.astype(np.int64)
    c = np.floor((x - lo) / side).astype(np.int64)
    return side, dims, (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]


def bucket_fps(x, k, bucket_size, max_cells=FPS_MAX_CELLS):
    """mgs_scan_fps: (indices, point-distance evaluations, buckets).  Per pick p
    a bucket with box [lo, hi] is visited when lb < its maximum of running
    minima, lb = (e0 e0 + e1 e1) + e2 e2, e = max(lo - p, p - hi, 0)"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    n = len(x)
    out = np.zeros(k, np.int32)
    if k <= 1:
        return out, 0, 0
    _, _, flat = bucket_grid(x, bucket_size, max_cells)
    order = np.argsort(flat, kind="stable")
    fs = flat[order]
    start = np.nonzero(np.concatenate([[True], fs[1:] != fs[:-1]]))[0]
    size = np.diff(np.concatenate([start, [n]]))
    of = np.repeat(np.arange(len(start)), size)          # bucket of each slot
    xs, orig = x[order], order.astype(np.int64)
    blo = np.minimum.reduceat(xs, start, axis=0)
    bhi = np.maximum.reduceat(xs, start, axis=0)
    dist = np.full(n, np.inf)
    bmax = np.full(len(start), np.inf)
    bidx = np.minimum.reduceat(orig, start)
    nevals = 0
    big = np.iinfo(np.int64).max
    for i in range(1, k):
        p = x[out[i - 1]]
        e = np.maximum(np.maximum(blo - p, p - bhi), 0.0)
        lb = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        visit = lb < bmax
        nevals += int(size[visit].sum())
        slots = np.nonzero(visit[of])[0]
        d = _dist(xs[slots], p)
        dist[slots] = np.where(d < dist[slots], d, dist[slots])
        bmax = np.maximum.reduceat(dist, start)
        bidx = np.minimum.reduceat(np.where(dist == bmax[of], orig, big), start)
        out[i] = int(bidx[bmax == bmax.max()].min())
    return out, nevals, len(start)


def cloud(S, cam_pos, cam_rot, width, height, fx, fy, cx, cy, extr, pfx, pfy, pcx, pcy, erode_iters, region, colors,
          voxel_size, num_points):
    """mgs_scan_cloud: (points float32, colors float32, dict(kept, voxels, evals))"""
    o, d = T.camera_rays(cam_pos, cam_rot, width, height, fx, fy, cx, cy)
    depth, seg, _, _ = T.render_bvh(S, o, d, (len(cam_pos), height, width))
    depth = depth.astype(np.float32).astype(np.float64)
    P, keep = T.points(depth, seg, extr, pfx, pfy, pcx, pcy, erode_iters, T.REGION if region is None else region)
    feat = np.asarray(colors, np.float32)[seg[keep]]
    V, F, _ = voxels(P[keep], feat, voxel_size)
    info = dict(kept=int(keep.sum()), voxels=len(V), evals=0)
    if len(V) >= num_points:
        idx, info["evals"], _ = bucket_fps(V.astype(np.float32).astype(np.float64), num_points, 8.0 * voxel_size)
        V, F = V[idx], F[idx]
    return V.astype(np.float32), F, info


# -- the clouds the host and GPU tests share -----------------------------------
def surface_cloud(n=4000, seed=3):
    """a plane and a sphere cap over it, float32-rounded like the CLI's pick input"""
    rng = np.random.default_rng(seed)
    m = n // 2
    plane = np.stack([rng.uniform(-0.25, 0.25, m), rng.uniform(-0.25, 0.25, m), np.zeros(m)], axis=1)
    u, phi = rng.uniform(0.3, 1.0, n - m), rng.uniform(0, 2 * np.pi, n - m)
    s = np.sqrt(1 - u * u)
    cap = 0.08 * np.stack([s * np.cos(phi), s * np.sin(phi), u], axis=1) + [0.03, -0.05, 0.0]
    x = np.concatenate([plane, cap])[rng.permutation(n)]
    return x.astype(np.float32).astype(np.float64)


def lattice(seed=4):
    """9 x 7 x 5 points at 2 mm spacing, every third one twice, shuffled: ties
    in every pick"""
    g = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3) * 0.002
    x = np.concatenate([g, g[::3]])
    return x[np.random.default_rng(seed).permutation(len(x))]


def boundary_values(b, rng, nrandom):
    """a >= 0 around the cell boundaries of size b: the multiples, their
    nextafter neighbours on both sides, random values"""
    k = np.arange(0, 60, dtype=np.float64)
    mult = np.concatenate([k * b, (k * 0.002), (k * 0.0123)])
    a = np.concatenate([mult, np.nextafter(mult, np.inf), np.nextafter(mult, -np.inf), rng.uniform(0, 60 * b, nrandom)])
    return a[a >= 0]


def adversarial_cloud(seed=7):
    """about 5 k points (f64) with float32 features: coordinates on and next
    to the cell boundaries of 0.002 and 0.0123, one 2 mm voxel holding 300
    points, duplicated points, the grid's anchor (0, 0, 0) among them"""
    rng = np.random.default_rng(seed)
    a = boundary_values(0.002, rng, 2000)
    a = a[a <= 0.125]
    P = np.stack([rng.choice(a, 3500), rng.choice(a, 3500), rng.choice(a, 3500)], axis=1)
    crowd = np.array([0.0501, 0.0701, 0.0301]) + rng.uniform(0, 0.0015, (300, 3))
    P = np.concatenate([np.zeros((1, 3)), P, crowd, P[:700], P[100:400]])
    P = P[rng.permutation(len(P))]
    F = rng.uniform(0, 1, (len(P), 3)).astype(np.float32)
    return P, F, rng.random(len(P)) > 0.3
