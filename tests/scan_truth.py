"""Plain-numpy restatement of the scene scan (csrc/mgs_scan.hip), the truth the
scan tests compare against.  Test infrastructure only.

Every dot product is written out as (a0 b0 + a1 b1) + a2 b2 -- no einsum, no
matmul in the arithmetic -- so the order of operations is the kernel's and the
results can be compared bit for bit.  Vectorised over rays only; each ray's own
sequence of operations is what one GPU lane executes.

  camera_rays     pixel-centre rays of a set of cameras
  render_brute    nearest hit by testing every triangle of every mesh, no BVH
  render_bvh      the threaded traversal, with its per-ray triangle-test counter
  erode           3 x 3 erosion with the outside counted as set
  points          erosion, back-projection, extrinsic and region crop
  point_tri_dist  distance from points to triangles (surface check)
  icosphere       subdivided icosahedron (a deep tree without a mesh file)
"""
import numpy as np

BOX, SPHERE, MESH = 0, 1, 2
INF = np.inf


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def camera_rays(cam_pos, cam_rot, width, height, fx, fy, cx, cy):
    """(origins, directions), (nview * height * width, 3) each, pixel order
    view, row, column: d = R ((c + 0.5 - cx) / fx, (r + 0.5 - cy) / fy, 1)"""
    cam_pos = np.asarray(cam_pos, np.float64).reshape(-1, 3)
    cam_rot = np.asarray(cam_rot, np.float64).reshape(-1, 3, 3)
    nv = len(cam_pos)
    r, c = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    dc0 = ((c + 0.5) - cx) / fx
    dc1 = ((r + 0.5) - cy) / fy
    o = np.empty((nv, height, width, 3))
    d = np.empty((nv, height, width, 3))
    for v in range(nv):
        R = cam_rot[v]
        for k in range(3):
            o[v, ..., k] = cam_pos[v, k]
            d[v, ..., k] = (R[k, 0] * dc0 + R[k, 1] * dc1) + R[k, 2]
    return o.reshape(-1, 3), d.reshape(-1, 3)


def ray_tri(o, d, T):
    """two-sided Moeller-Trumbore, the expressions of ray_tri in
    csrc/mgs_sampler.hip; o, d (..., 3), T (..., 9) broadcast: (hit, t)"""
    v0, v1, v2 = T[..., 0:3], T[..., 3:6], T[..., 6:9]
    e1, e2 = v1 - v0, v2 - v0
    p0 = d[..., 1] * e2[..., 2] - d[..., 2] * e2[..., 1]
    p1 = d[..., 2] * e2[..., 0] - d[..., 0] * e2[..., 2]
    p2 = d[..., 0] * e2[..., 1] - d[..., 1] * e2[..., 0]
    det = (e1[..., 0] * p0 + e1[..., 1] * p1) + e1[..., 2] * p2
    ok = np.abs(det) > 1e-12
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / det
        tv = o - v0
        u = ((tv[..., 0] * p0 + tv[..., 1] * p1) + tv[..., 2] * p2) * inv
        q0 = tv[..., 1] * e1[..., 2] - tv[..., 2] * e1[..., 1]
        q1 = tv[..., 2] * e1[..., 0] - tv[..., 0] * e1[..., 2]
        q2 = tv[..., 0] * e1[..., 1] - tv[..., 1] * e1[..., 0]
        w = ((q0 * d[..., 0] + q1 * d[..., 1]) + q2 * d[..., 2]) * inv
        t = ((e2[..., 0] * q0 + e2[..., 1] * q1) + e2[..., 2] * q2) * inv
        hit = ok & (u >= 0.0) & (w >= 0.0) & (u + w <= 1.0) & (t > 0.0)
    return hit, t


def slab(o, d, inv, lo, hi):
    """scan_slab: (meets, entry, exit); a zero direction component is an inside
    test of that axis"""
    n = len(o)
    tnear, tfar, miss = np.full(n, -INF), np.full(n, INF), np.zeros(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            zero = d[:, k] == 0.0
            miss |= zero & ((o[:, k] < lo[..., k]) | (o[:, k] > hi[..., k]))
            a = (lo[..., k] - o[:, k]) * inv[:, k]
            b = (hi[..., k] - o[:, k]) * inv[:, k]
            mn = np.where(a < b, a, b)
            mx = np.where(a < b, b, a)
            tnear = np.where(~zero & (mn > tnear), mn, tnear)
            tfar = np.where(~zero & (mx < tfar), mx, tfar)
    return ~miss & (tnear <= tfar), tnear, tfar


def to_frame(o, d, pos, R):
    """the ray in a geom frame: R^T (o - pos), R^T d, and 1 / direction"""
    v = o - pos
    om, dm = np.empty_like(o), np.empty_like(d)
    for k in range(3):
        om[:, k] = (R[0, k] * v[:, 0] + R[1, k] * v[:, 1]) + R[2, k] * v[:, 2]
        dm[:, k] = (R[0, k] * d[:, 0] + R[1, k] * d[:, 1]) + R[2, k] * d[:, 2]
    with np.errstate(divide="ignore"):
        inv = 1.0 / dm
    return v, om, dm, inv


class _Best:
    def __init__(self, n):
        self.t = np.full(n, INF)
        self.draw = np.full(n, -1, np.int64)
        self.seg = np.full(n, -1, np.int32)
        self.face = np.full(n, -1, np.int32)
        self.ntest = np.zeros(n, np.int32)

    def take(self, rows, t, di, seg, face):
        self.t[rows], self.draw[rows], self.seg[rows], self.face[rows] = t, di, seg, face

    def images(self, shape):
        depth = np.where(self.draw >= 0, self.t, 0.0)
        return depth.reshape(shape), self.seg.reshape(shape), self.face.reshape(shape), self.ntest.reshape(shape)


def _primitive(S, j, o, d, best):
    """box or sphere drawable j; returns False for a mesh"""
    kind, pos, R, size = int(S["draw_type"][j]), S["draw_pos"][j], S["draw_rot"][j].reshape(3, 3), S["draw_size"][j]
    if kind == MESH:
        return False
    v, om, dm, inv = to_frame(o, d, pos, R)
    if kind == SPHERE:
        a, b = dot3(d, d), dot3(v, d)
        c = dot3(v, v) - size[0] * size[0]
        disc = b * b - a * c
        with np.errstate(invalid="ignore"):
            s = np.sqrt(disc)
            t0, t1 = (-b - s) / a, (-b + s) / a
            t = np.where(t0 > 0.0, t0, t1)
            ok = (disc >= 0.0) & (t > 0.0) & (t < best.t)
    else:
        meets, tn, tf = slab(om, dm, inv, -size, size)
        t = np.where(tn > 0.0, tn, tf)
        ok = meets & (t > 0.0) & (t < best.t)
    rows = np.nonzero(ok)[0]
    best.take(rows, t[rows], j, S["draw_id"][j], -1)
    return True


def render_brute(S, o, d, shape, chunk=256):
    """every triangle of every mesh instance against every ray: the nearest hit
    as the lexicographic minimum of (t, drawable index, face id)"""
    best = _Best(len(o))
    for j in range(len(S["draw_type"])):
        if _primitive(S, j, o, d, best):
            continue
        m = int(S["draw_mesh"][j])
        t0, t1 = int(S["mesh_tri0"][m]), int(S["mesh_tri0"][m + 1])
        if t1 == t0:
            continue
        T, F = S["tri"].reshape(-1, 9)[t0:t1], S["tri_face"][t0:t1]
        _, om, dm, _ = to_frame(o, d, S["draw_pos"][j], S["draw_rot"][j].reshape(3, 3))
        for a in range(0, len(o), chunk):
            rows = np.arange(a, min(a + chunk, len(o)))
            hit, t = ray_tri(om[rows, None, :], dm[rows, None, :], T[None, :, :])
            t = np.where(hit, t, INF)
            tmin = t.min(axis=1)
            face = np.where(t == tmin[:, None], F[None, :], np.iinfo(np.int32).max).min(axis=1)
            ok = np.isfinite(tmin) & (tmin < best.t[rows])
            best.take(rows[ok], tmin[ok], j, S["draw_id"][j], face[ok])
    return best.images(shape)[:3]


def render_bvh(S, o, d, shape):
    """the kernel's walk of the threaded BVH, every ray at its own node:
    (depth, seg, tri, ntest)"""
    best = _Best(len(o))
    box, skip = S["node_box"].reshape(-1, 6), S["node_skip"]
    first, count = S["node_first"], S["node_count"]
    tri, face = S["tri"].reshape(-1, 9), S["tri_face"]
    for j in range(len(S["draw_type"])):
        if _primitive(S, j, o, d, best):
            continue
        m = int(S["draw_mesh"][j])
        node0, nnode = int(S["mesh_node0"][m]), int(S["mesh_node0"][m + 1] - S["mesh_node0"][m])
        tri0 = int(S["mesh_tri0"][m])
        _, om, dm, inv = to_frame(o, d, S["draw_pos"][j], S["draw_rot"][j].reshape(3, 3))
        i = np.zeros(len(o), np.int64)
        while True:
            rows = np.nonzero(i < nnode)[0]
            if len(rows) == 0:
                break
            g = node0 + i[rows]
            meets, tn, tf = slab(om[rows], dm[rows], inv[rows], box[g, :3], box[g, 3:])
            with np.errstate(invalid="ignore"):
                enter = meets & (tf >= 0.0) & (tn <= best.t[rows])
            cnt = np.where(enter, count[g], 0)
            for q in range(int(cnt.max(initial=0))):
                sel = np.nonzero(cnt > q)[0]
                rr, k = rows[sel], tri0 + first[g[sel]] + q
                best.ntest[rr] += 1
                hit, t = ray_tri(om[rr], dm[rr], tri[k])
                f = face[k]
                better = hit & ((t < best.t[rr]) | ((t == best.t[rr]) & (best.draw[rr] == j) & (f < best.face[rr])))
                best.take(rr[better], t[better], j, S["draw_id"][j], f[better])
            i[rows] = np.where(enter & (count[g] == 0), i[rows] + 1, skip[g])
    return best.images(shape)


def erode(mask, iterations):
    """(..., H, W) bool, eroded `iterations` times by a 3 x 3 square; pixels
    outside the image count as set"""
    m = np.asarray(mask, bool).copy()
    h, w = m.shape[-2:]
    for _ in range(iterations):
        p = np.ones(m.shape[:-2] + (h + 2, w + 2), bool)
        p[..., 1:-1, 1:-1] = m
        m = np.ones_like(m)
        for dr in (0, 1, 2):
            for dc in (0, 1, 2):
                m = m & p[..., dr:dr + h, dc:dc + w]
    return m


REGION = np.array([-0.25, -0.25, -0.01, 0.25, 0.25, 1.0])


def points(depth, seg, extr, fx, fy, cx, cy, iterations, region=REGION):
    """mgs_scan_points: (points (nview, H, W, 3), keep (nview, H, W))"""
    nv, h, w = depth.shape
    r, c = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    z = depth
    x = ((c - cx) * z) / fx
    y = ((r - cy) * z) / fy
    E = np.asarray(extr, np.float64).reshape(nv, 4, 4)
    P = np.empty((nv, h, w, 3))
    for k in range(3):
        e = E[:, k, :, None, None]
        P[..., k] = ((e[:, 0] * x + e[:, 1] * y) + e[:, 2] * z) + e[:, 3]
    inside = np.ones((nv, h, w), bool)
    for k in range(3):
        inside &= (P[..., k] > region[k]) & (P[..., k] < region[3 + k])
    return P, erode(seg != -1, iterations) & inside


def point_tri_dist(p, T):
    """distance from points p (n, 3) to triangles T (n, 3, 3), row by row
    (closest point by clamping the barycentric regions, Ericson 5.1.5)"""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = np.sum(ab * ap, 1), np.sum(ac * ap, 1)
    bp = p - b
    d3, d4 = np.sum(ab * bp, 1), np.sum(ac * bp, 1)
    cp = p - c
    d5, d6 = np.sum(ab * cp, 1), np.sum(ac * cp, 1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        den = 1.0 / (va + vb + vc)
        v, w = vb * den, vc * den
        q = a + ab * v[:, None] + ac * w[:, None]                                   # interior
        e_ab = a + ab * (d1 / (d1 - d3))[:, None]
        e_ac = a + ac * (d2 / (d2 - d6))[:, None]
        e_bc = b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None]
    out = q
    cond = [((d1 <= 0) & (d2 <= 0), a), ((d3 >= 0) & (d4 <= d3), b), ((d6 >= 0) & (d5 <= d6), c),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), e_ab), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), e_ac),
            ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), e_bc)]
    done = np.zeros(len(p), bool)
    for m, val in cond:
        take = m & ~done
        out = np.where(take[:, None], val, out)
        done |= m
    return np.linalg.norm(p - out, axis=1)


def icosphere(subdiv, radius=1.0):
    """(verts, faces) of an icosahedron subdivided `subdiv` times (20 * 4^subdiv
    faces), vertices on the sphere"""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius, np.array(f, np.int64)


# -- the scenes the host and GPU tests share ---------------------------------
def rot(axis, angle):
    """rotation matrix about a (normalised here) axis, Rodrigues"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


ONE_TRIANGLE = (np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.02], [0.0, 0.1, 0.05]]), np.array([[0, 1, 2]]))
SEVEN_TRIANGLES = (np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0.3], [3, 0, 0], [0, 1, 0], [1, 1, 0.2], [2, 1, 0], [3, 1, 0.1],
                             [1.5, 2, 0]]) * 0.03,
                   np.array([[0, 1, 4], [1, 5, 4], [1, 2, 5], [2, 6, 5], [2, 3, 6], [3, 7, 6], [5, 6, 8]]))


def shipped_mesh(dataset, object_id, file_name):
    from mgs.core.mjcf import load_mesh_bytes
    from mgs.util.const import ASSET_PATH
    import os
    path = os.path.join(ASSET_PATH, "mj-objects", dataset, object_id, file_name)
    with open(path, "rb") as f:
        return load_mesh_bytes(f.read(), path)


def fibonacci_cameras(num, which=None):
    """(pos (n, 3), rot (n, 3, 3) OpenCV axes) of the clutter scan's views"""
    from mgs.scan.scene import look_at_frame
    from mgs.util.camera import fibonacci_sphere
    pos, R = [], []
    for i in (range(num) if which is None else which):
        p = fibonacci_sphere(num, i)
        p[2] = abs(p[2]) + 0.01
        F = look_at_frame(p, [0.0, 0.0, -0.025])
        pos.append(p)
        R.append(np.stack([F[:, 0], -F[:, 1], -F[:, 2]], axis=1))
    return np.array(pos), np.array(R)


def small_scene():
    """table box, a sphere, the orange, the mug twice (one BVH, two rotated
    poses), a 1-triangle mesh; seg ids 10 .. 15 (not the drawable indices)"""
    from mgs.scan.scene import ScanScene
    sc = ScanScene()
    sc.add_box(10, [0.0, 0.0, -0.02], None, [10.0, 10.0, 0.02])
    sc.add_sphere(11, [0.1, -0.08, 0.03], 0.03)
    v, f = shipped_mesh("YCB", "017_orange", "textured.obj")
    sc.add_mesh(12, [0.0, 0.0, 0.04], rot([1, 2, 3], 0.7), v, f, key="orange")
    v, f = shipped_mesh("GoogleScannedObjects", "Synthetic_Mug_Body", "model.obj")
    sc.add_mesh(13, [-0.12, 0.05, 0.06], rot([0, 1, 0], 1.1), v, f, key="mug")
    sc.add_mesh(14, [0.08, 0.12, 0.05], rot([1, -1, 0.5], 2.3), key="mug")
    sc.add_mesh(15, [-0.05, -0.15, 0.05], rot([0, 0, 1], 0.4), *ONE_TRIANGLE, key="one")
    return sc


def small_cameras():
    """the three Fibonacci views of num_images = 3 (two of them the low camera
    at z = 0.01, whose upper rays miss everything) and one camera inside the
    table box"""
    from mgs.scan.scene import look_at_frame
    pos, R = fibonacci_cameras(3)
    inside = np.array([0.3, 0.2, -0.03])
    F = look_at_frame(inside, [0.0, 0.0, -0.025])
    return np.concatenate([pos, inside[None]]), np.concatenate([R, np.stack([F[:, 0], -F[:, 1], -F[:, 2]], 1)[None]])


def focal(height, fovy=45.0):
    return (height / 2) / np.tan(fovy * np.pi / 360)


def truth(S, cam_pos, cam_rot, width, height):
    """dict(depth, seg, tri, ntest from the traversal; brute = (depth, seg, tri))"""
    f = focal(height)
    o, d = camera_rays(cam_pos, cam_rot, width, height, f, f, width / 2, height / 2)
    shape = (len(cam_pos), height, width)
    depth, seg, tri, ntest = render_bvh(S, o, d, shape)
    return dict(depth=depth, seg=seg, tri=tri, ntest=ntest, brute=render_brute(S, o, d, shape))
