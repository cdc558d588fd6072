"""Truth for the capsule and cylinder drawables of the scene scan (scan_rod in
csrc/mgs_scan.hip) and for the gripper scan built on them.  Test infrastructure
only; numpy, independent of the package.

  rod             the two ray tests in the kernel's order of operations
  render_brute /  scan_truth's renderers with the two types plugged in
  render_bvh / truth
  sdf_capsule /   exact signed distances, and a sphere-tracing marcher over
  sdf_cylinder /  them: a first hit that uses none of the quadratic formulas
  march
"""
import contextlib

import numpy as np

import scan_truth as T

CAPSULE, CYLINDER = 3, 4
INF = np.inf


def rod(om, dm, r, h, cyl):
    """scan_rod: smallest t > 0 at which the rays om + t dm (n, 3; geom frame)
    meet a capsule (cyl False) or a capped cylinder of radius r, half-length h
    about z; inf where none"""
    om, dm = np.asarray(om, np.float64), np.asarray(dm, np.float64)
    n = len(om)
    t = np.full(n, INF)
    rr = r * r
    o0, o1, o2, d0, d1, d2 = om[:, 0], om[:, 1], om[:, 2], dm[:, 0], dm[:, 1], dm[:, 2]

    def take(t, cand, ok):
        with np.errstate(invalid="ignore"):
            return np.where(ok & (cand > 0.0) & (cand < t), cand, t)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = d0 * d0 + d1 * d1
        b = o0 * d0 + o1 * d1
        c = (o0 * o0 + o1 * o1) - rr
        disc = b * b - a * c
        side = (a > 0.0) & (disc >= 0.0)
        s = np.sqrt(disc)
        for tk in ((-b - s) / a, (-b + s) / a):
            t = take(t, tk, side & (np.abs(o2 + tk * d2) <= h))
        if cyl:
            for e in (h, -h):
                tc = (e - o2) / d2
                x, y = o0 + tc * d0, o1 + tc * d1
                t = take(t, tc, (d2 != 0.0) & ((x * x + y * y) <= rr))
            return t
        A = a + d2 * d2
        for sg in (1.0, -1.0):
            w = o2 - sg * h
            B = (o0 * d0 + o1 * d1) + w * d2
            C = ((o0 * o0 + o1 * o1) + w * w) - rr
            disc = B * B - A * C
            s = np.sqrt(disc)
            for tk in ((-B - s) / A, (-B + s) / A):
                t = take(t, tk, (disc >= 0.0) & (sg * (w + tk * d2) >= 0.0))
    return t


def _primitive(S, j, o, d, best, _base=T._primitive):
    """scan_truth._primitive with the capsule and cylinder branches"""
    kind = int(S["draw_type"][j])
    if kind not in (CAPSULE, CYLINDER):
        return _base(S, j, o, d, best)
    _, om, dm, _ = T.to_frame(o, d, S["draw_pos"][j], S["draw_rot"][j].reshape(3, 3))
    size = S["draw_size"][j]
    t = rod(om, dm, size[0], size[1], kind == CYLINDER)
    rows = np.nonzero(t < best.t)[0]
    best.take(rows, t[rows], j, S["draw_id"][j], -1)
    return True


@contextlib.contextmanager
def _plugged():
    old = T._primitive
    T._primitive = _primitive
    try:
        yield
    finally:
        T._primitive = old


def render_brute(S, o, d, shape, chunk=256):
    with _plugged():
        return T.render_brute(S, o, d, shape, chunk)


def render_bvh(S, o, d, shape):
    with _plugged():
        return T.render_bvh(S, o, d, shape)


def truth(S, cam_pos, cam_rot, width, height):
    with _plugged():
        return T.truth(S, cam_pos, cam_rot, width, height)


# -- exact distances and a marcher -------------------------------------------------
def sdf_capsule(p, r, h):
    q = p.copy()
    q[:, 2] = p[:, 2] - np.clip(p[:, 2], -h, h)
    return np.linalg.norm(q, axis=1) - r


def sdf_cylinder(p, r, h):
    dx = np.hypot(p[:, 0], p[:, 1]) - r
    dz = np.abs(p[:, 2]) - h
    return np.minimum(np.maximum(dx, dz), 0.0) + np.hypot(np.maximum(dx, 0.0), np.maximum(dz, 0.0))


def march(sdf, o, u, hit_eps=1e-13, far=3.0, max_iter=4000):
    """sphere tracing of the rays o + t u (u unit) from outside: (t where the
    distance fell below hit_eps, else inf; the smallest distance seen)"""
    n = len(o)
    t = np.zeros(n)
    tmin = np.full(n, INF)
    hit = np.full(n, INF)
    live = np.ones(n, bool)
    for _ in range(max_iter):
        rows = np.nonzero(live)[0]
        if len(rows) == 0:
            break
        dist = sdf(o[rows] + t[rows, None] * u[rows])
        tmin[rows] = np.minimum(tmin[rows], dist)
        got = dist < hit_eps
        hit[rows[got]] = t[rows[got]]
        t[rows] = t[rows] + dist
        live[rows[got]] = False
        live[rows[~got & (t[rows] > far)]] = False
    return hit, tmin


def random_rays(n, reach, seed):
    """origins on the unit sphere, unit directions toward points of the box
    [-reach, reach]^3"""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o /= np.linalg.norm(o, axis=1, keepdims=True)
    u = rng.uniform(-reach, reach, size=(n, 3)) - o
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return o, u
