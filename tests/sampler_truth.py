"""Independent truths of the grasp-candidate samplers (csrc/mgs_sampler.hip,
csrc/mgs_contact.hip), the references the sampler tests compare the kernels and
the C oracle against.  Test infrastructure only; imports neither the oracle nor
the engine.

  ray_contacts        the ray caster in plain numpy float64, in the kernel's
                      order of operations (bit for bit)
  ray_contacts_exact  the same rule in fractions.Fraction on the float inputs,
                      with every ray's distance from a decision
  nested_shells       three nested icospheres, 720 triangles, optionally shuffled
  shell_rays          rays from spheres between, outside and inside the shells
  dyadic_box          a box and rays on which every intermediate is exact
  u_sweep             choice uniforms at every slot edge of every ray
  seeds               nearest seed and the ntip largest splitmix64 keys
  seed_lattice        seeds on a 0.125 lattice: duplicates, distances == radius
  fit                 the AdamW fit: torch float64 transcription of the
                      reference's formulas, gradient by autograd, AdamW and the
                      joint clip in numpy; batched over candidates
  fit_case            candidates drawn as the GPU parity test draws them
  fit_reference       the fit truth the CPU and GPU tests share, computed once
  check_fit           the comparison of an implementation with that truth

The farthest-point pick's truth is cloud_truth.brute_fps.
"""
from fractions import Fraction
from functools import lru_cache
from itertools import permutations

import numpy as np
import torch

import scan_truth as T

# ---------------------------------------------------------------------------
# rays


def _valid_hits(tri, o, d, eps):
    """(valid (n, m), location (n, m, 3)) of the rays o + t d against every
    triangle: ray_tri, then loc = o + t d and sqrt(sum (loc - o)^2) >= eps"""
    hit, t = T.ray_tri(o[:, None, :], d[:, None, :], tri[None, :, :])
    with np.errstate(invalid="ignore", over="ignore"):
        loc = o[:, None, :] + t[..., None] * d[:, None, :]
        r = loc - o[:, None, :]
        s = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        valid = hit & (np.sqrt(s) >= eps)
    return valid, loc


def ray_contacts(tri, origin, direction, u, eps):
    """mgs_antipodal_kernel: (second (n, 3), nvalid (n,) int32).  The valid hits
    of +d by triangle index, then those of -d by triangle index; of these
    `total` hits the k-th, k = min(floor(u * total), total - 1), zeros without
    a hit.  u in [0, 1]."""
    tri = np.asarray(tri, np.float64).reshape(-1, 9)
    o = np.asarray(origin, np.float64).reshape(-1, 3)
    d = np.asarray(direction, np.float64).reshape(-1, 3)
    u = np.asarray(u, np.float64).reshape(-1)
    n = len(o)
    if n > 512:                                                # bound the (rays, triangles) temporaries
        parts = [ray_contacts(tri, o[a:a + 512], d[a:a + 512], u[a:a + 512], eps) for a in range(0, n, 512)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    vp, lp = _valid_hits(tri, o, d, eps)
    vm, lm = _valid_hits(tri, o, -d, eps)
    valid = np.concatenate([vp, vm], axis=1)
    loc = np.concatenate([lp, lm], axis=1)
    total = valid.sum(axis=1)
    fk = np.floor(u * total.astype(np.float64))
    kth = np.where(fk < (total - 1).astype(np.float64), fk, total - 1).astype(np.int64)
    second = np.zeros((n, 3))
    if valid.shape[1]:
        rank = np.cumsum(valid, axis=1) - 1                  # rank of each valid hit in the list
        pick = valid & (rank == kth[:, None])
        has = pick.any(axis=1)
        col = np.argmax(pick, axis=1)
        second[has] = loc[np.nonzero(has)[0], col[has]]
    return second, total.astype(np.int32)


# exact side: a triangle whose float barycentrics lie this far outside [0, 1]
# (with a determinant this far from 0) is a miss without exact arithmetic.  The
# float error of u, w is below 1e-9 there (a few ulps of O(1) products over a
# determinant above 1e-6), five orders below the margin.
_CULL, _CULL_DET = 1e-2, 1e-6


def _fr3(a):
    return [Fraction(float(x)) for x in a]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def ray_contacts_exact(tri, origin, direction, u, eps):
    """The rule of ray_contacts in exact rational arithmetic on the float
    inputs: a triangle is hit when det != 0, u >= 0, w >= 0, u + w <= 1, t > 0;
    the hit counts when |t d| >= eps; of the `total` hits (+d by triangle index,
    then -d) the k-th, k = min(floor(u * total), total - 1).

    Returns (second (n, 3) -- the exact point rounded once to float64, nvalid
    (n,), margin (n,)).  margin is the ray's distance from a decision: the
    smallest change of a barycentric coordinate, of t, of the hit distance
    against eps, of a determinant against 0 or of u * total against an integer
    that would alter the answer."""
    tri = np.asarray(tri, np.float64).reshape(-1, 9)
    o = np.asarray(origin, np.float64).reshape(-1, 3)
    d = np.asarray(direction, np.float64).reshape(-1, 3)
    u = np.asarray(u, np.float64).reshape(-1)
    n = len(o)
    second, nvalid, margin = np.zeros((n, 3)), np.zeros(n, np.int32), np.full(n, np.inf)
    # float barycentrics, only to leave far-away triangles out (see _CULL)
    v0, e1, e2 = tri[:, 0:3], tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
    feps2 = Fraction(float(eps)) ** 2
    triF = [[_fr3(t[0:3]), _fr3(t[3:6]), _fr3(t[6:9])] for t in tri]
    for i in range(n):
        if len(tri):
            p = np.cross(d[i], e2)
            det = np.einsum("ij,ij->i", e1, p)
            with np.errstate(divide="ignore", invalid="ignore"):
                tv = o[i] - v0
                fu = np.einsum("ij,ij->i", tv, p) / det
                fw = np.einsum("ij,j->i", np.cross(tv, e1), d[i]) / det
                far = (np.abs(det) > _CULL_DET) & ((fu < -_CULL) | (fw < -_CULL) | (fu + fw > 1.0 + _CULL))
            near = np.nonzero(~far)[0]
        else:
            near = []
        oF, dF = _fr3(o[i]), _fr3(d[i])
        dd = _dot(dF, dF)
        hits = ([], [])                                       # (+d, -d): exact t of the valid hits
        m = _CULL if len(near) < len(tri) else np.inf         # margins are resolved below _CULL only
        for j in near:
            a, b, c = triF[j]
            E1 = [b[k] - a[k] for k in range(3)]
            E2 = [c[k] - a[k] for k in range(3)]
            P = _cross(dF, E2)
            D = _dot(E1, P)
            if D == 0:
                continue                                      # parallel: exactly no hit, and far from one
            TV = [oF[k] - a[k] for k in range(3)]
            U = _dot(TV, P) / D
            Q = _cross(TV, E1)
            W = _dot(Q, dF) / D
            Tt = _dot(E2, Q) / D
            slack = [U, W, 1 - U - W]
            dist2 = Tt * Tt * dd
            inside = min(slack) >= 0
            if inside and Tt != 0 and dist2 >= feps2:
                hits[0 if Tt > 0 else 1].append(Tt)
            # how far this triangle is from changing the count
            bad = [-float(s) for s in slack if s < 0]
            if Tt == 0:
                bad.append(0.0)
            gap = abs(np.sqrt(float(dist2)) - float(eps))
            if dist2 < feps2:
                bad.append(gap)
            own = max(bad) if bad else min([float(s) for s in slack] + [abs(float(Tt)), gap, abs(float(D))])
            m = min(m, own)
        total = len(hits[0]) + len(hits[1])
        nvalid[i] = total
        if total:
            x = Fraction(float(u[i])) * total
            k = min(int(x // 1), total - 1)
            tk = (hits[0] + hits[1])[k]
            second[i] = [float(oF[c] + tk * dF[c]) for c in range(3)]
            if float(u[i]) < 1.0:
                fx = float(x - (x // 1))
                m = min(m, fx if k > 0 else np.inf, 1.0 - fx if k < total - 1 else np.inf)
        margin[i] = m
    return second, nvalid, margin


def nested_shells(shuffled=False, seed=11):
    """(720, 9): icospheres of radius 1.0 (320 triangles), 0.6 (320) and 0.3 (80)
    one inside the other; shuffled: the rows permuted by a fixed seed, so that
    the hits of one ray lie in different tiles of 256, out of depth order"""
    parts = []
    for subdiv, radius in ((2, 1.0), (2, 0.6), (1, 0.3)):
        v, f = T.icosphere(subdiv, radius)
        parts.append(v[f].reshape(-1, 9))
    tri = np.concatenate(parts)
    if shuffled:
        tri = tri[np.random.default_rng(seed).permutation(len(tri))]
    return np.ascontiguousarray(tri)


def shell_rays(n=600, seed=12):
    """(origin, direction, u): rays from spheres of radius 1.2, 0.8, 0.45 and
    0.1 (outside, between and inside the shells) in uniform unit directions"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    o = p * np.array([1.2, 0.8, 0.45, 0.1])[np.arange(n) % 4][:, None]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d, rng.random(n)


def dyadic_box():
    """(tri (12, 9), origin, direction, u): a box of half sizes 0.5, 0.25, 0.125
    and rays with dyadic origins and directions whose components are 0 or powers
    of two -- every determinant is a power of two and every intermediate of
    ray_tri is exact in float64.  The faces' centres lie on their diagonals,
    which on the x and z faces are the edge v1 v2 of one triangle (u + w == 1)
    and the edge v0 v1 of the other (w == 0), on the y faces the edge v0 v2 of
    both (u == 0)."""
    h = np.array([0.5, 0.25, 0.125])
    v = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64) * h
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = []
    for q, (a, b, c, e) in enumerate(quads):
        f += [(a, b, c), (c, e, a)] if q in (2, 3) else [(b, c, a), (a, c, e)]
    tri = v[np.array(f)].reshape(-1, 9)
    rays = []                                                  # (origin, direction)
    axes = np.eye(3)
    for k in range(3):                                         # through face centres
        rays += [(np.zeros(3), axes[k]), (2.0 * axes[k], -axes[k]), (-2.0 * axes[k], axes[k])]
        rays += [(h[k] * axes[k], axes[k]), (h[k] * axes[k], -axes[k])]       # from a face's centre
    for a, b in ((0, 1), (0, 2), (1, 2)):                      # through edge midpoints
        for sa in (1, -1):
            e = sa * h[a] * axes[a] + h[b] * axes[b]
            rays += [(np.zeros(3), e), (3.0 * e, -e)]
    for sx in (1, -1):                                         # through corners
        for sy in (1, -1):
            c = np.array([sx, sy, 1.0]) * h
            rays += [(np.zeros(3), c), (2.0 * c, -c), (np.array([0.0, 0.0, c[2]]), np.array([c[0], c[1], 0.0]))]
    rays += [(np.array([-1.0, 0.25, 0.0]), axes[0]),           # along the face y = 0.25
             (np.array([-1.0, 0.25, 0.0625]), axes[0]),
             (np.array([0.25, -1.0, 0.125]), axes[1]),         # along the face z = 0.125
             (np.array([0.0, 0.0, 0.125]), np.array([1.0, 0.5, 0.0])),     # in a face, to its corner
             (np.array([0.5, 0.0625, 0.03125]), axes[0]),      # from points on a face
             (np.array([0.5, 0.0625, 0.03125]), np.array([-1.0, 0.5, 0.25])),
             (np.array([0.125, 0.25, -0.0625]), np.array([1.0, -1.0, 0.5])),
             (np.array([0.125, 0.0625, 0.03125]), np.array([1.0, 1.0, 1.0])),  # generic, inside
             (np.array([0.125, 0.0625, 0.03125]), np.array([-2.0, 1.0, 0.5])),
             (np.array([-0.375, 0.125, -0.0625]), np.array([0.5, 0.25, -1.0])),
             (np.array([1.0, 1.0, 1.0]), np.array([1.0, 0.0, 0.0])),          # misses
             (np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 1.0]))]
    o = np.array([r[0] for r in rays], np.float64)
    d = np.array([r[1] for r in rays], np.float64)
    u = (np.arange(len(o)) * 3 % 8) / 8.0                      # u * total is exact
    return tri, o, d, u


def u_sweep(nvalid):
    """(ray index, u) lists that put, for every slot j of every ray with hits,
    the choice uniform at the slot's edges: j / total, the double below it, the
    slot's middle, 0, the double below 1 and exactly 1, cycling"""
    idx, us = [], []
    q = 0
    for i, total in enumerate(np.asarray(nvalid)):
        for j in range(int(total)):
            e = j / float(total)
            cand = (e, np.nextafter(e, -1.0) if j else 0.0, (j + 0.5) / float(total), 0.0, np.nextafter(1.0, 0.0), 1.0)
            for c in (cand[q % 6], cand[(q + 1) % 6]):
                idx.append(i)
                us.append(c)
            q += 2
    return np.array(idx, np.int64), np.array(us, np.float64)


# ---------------------------------------------------------------------------
# seeds
_M64 = (1 << 64) - 1


def splitmix64_int(x):
    """splitmix64 (Steele, Lea, Flood 2014) in Python integers"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def key_uniform_int(seed, ctr):
    return (splitmix64_int((seed & _M64) ^ splitmix64_int(ctr)) >> 11) / 9007199254740992.0


def _splitmix64(x):
    """the same on uint64 arrays (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def key_uniforms(seed, k):
    """(k, k): the key of the pair (i, j) is the uniform of counter i * k + j"""
    ctr = np.arange(k * k, dtype=np.uint64).reshape(k, k)
    bits = _splitmix64(np.uint64(seed & _M64) ^ _splitmix64(ctr))
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def seeds(S, radius, key, ntip):
    """mgs_seeds_kernel: (nn (k,), sel (k, ntip)).  nn[i]: the second of the
    seeds sorted by (distance from i, index), the seed itself when it is alone.
    sel[i]: the last ntip of the seeds sorted by (key, index), the key -inf
    unless distance < radius; with fewer than ntip seeds, all of them in that
    order and then the seed itself."""
    S = np.asarray(S, np.float64).reshape(-1, 3)
    k = len(S)
    df = S[None, :, :] - S[:, None, :]
    dist = np.sqrt((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2])
    order = np.argsort(dist, axis=1, kind="stable")
    nn = order[:, 1] if k > 1 else order[:, 0]
    keys = np.where(dist < radius, key_uniforms(key, k), -np.inf)
    ranked = np.argsort(keys, axis=1, kind="stable")[:, -ntip:]
    if k < ntip:
        ranked = np.concatenate([ranked, np.repeat(np.arange(k)[:, None], ntip - k, axis=1)], axis=1)
    return nn.astype(np.int32), ranked.astype(np.int32)


SEED_K = (1, 2, 4, 5, 255, 256, 257, 513)
SEED_NTIP = (1, 3, 5)
SEED_RADIUS = (0.0, 1e-9, 0.125, 10.0)
SEED_KEY = (0, 99, 2**63 + 12345, 2**64 - 1)


def seed_lattice(k, seed=21):
    """k seeds on a lattice of pitch 0.125 with six cells a side: duplicates
    (the second seed repeats the first) and distances exactly 0.125"""
    s = np.random.default_rng(seed + k).integers(0, 6, size=(k, 3)).astype(np.float64) * 0.125
    if k > 1:
        s[1] = s[0]
    return s


# ---------------------------------------------------------------------------
# the fit: the reference's formulas (mgs/sampler/kin/jax_util.py, kin/base.py
# forward_kinematic_point_transform, sampler/contact.py update / loss_fn) in
# torch float64; optax.adamw(0.005) and the joint clip in numpy
LR, B1, B2, ADAM_EPS, WEIGHT_DECAY, COS_WEIGHT = 0.005, 0.9, 0.999, 1e-8, 1e-4, 0.001


def _qmul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def _qapply(q, p):
    pq = torch.cat((torch.zeros_like(p[..., :1]), p), -1)
    return _qmul(_qmul(q, pq), q * q.new_tensor([1.0, -1.0, -1.0, -1.0]))[..., 1:]


def _se3_mul(A, B):
    return torch.cat((_qmul(A[..., :4], B[..., :4]), _qapply(A[..., :4], B[..., 4:]) + A[..., 4:]), -1)


def _rot6(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = a1 / torch.linalg.norm(a1, dim=-1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / torch.linalg.norm(b2, dim=-1, keepdim=True)
    return torch.stack((b1, b2, torch.linalg.cross(b1, b2)), -2)


def _tip_frames(kin, theta):
    """world (hand-frame) transforms (B, ntip, 7) of the fingertip links"""
    B = theta.shape[0]
    par = kin.parents()
    ident = theta.new_tensor([1.0, 0, 0, 0, 0, 0, 0]).expand(B, 7)
    links = [ident]
    for i in range(kin.num_dofs):
        jt = theta.new_tensor(kin.joint_tf[i])
        axis = jt[3:] / torch.linalg.norm(jt[3:])
        half = theta[:, i] / 2.0
        s = torch.sin(half)
        quat = torch.stack((torch.cos(half), axis[0] * s, axis[1] * s, axis[2] * s), -1)
        dyn = torch.cat((quat, jt[:3] * theta[:, i:i + 1]), -1)
        static = theta.new_tensor(kin.kin_tf[i]).expand(B, 7)
        links.append(_se3_mul(_se3_mul(links[par[i] + 1], static), dyn))
    return torch.stack([links[int(t) + 1] for t in kin.fingertip_idx], 1)


def _assign(pos, targets, perms):
    """find_best_assignment_and_reorder_targets: (targets reordered, the gap
    between the least and the second-least summed distance)"""
    D = torch.sqrt(((pos[:, :, None, :] - targets[:, None, :, :]) ** 2).sum(-1))
    cost = D[:, torch.arange(pos.shape[1]), perms].sum(-1)             # (B, nperm)
    low = torch.sort(cost, dim=1).values
    best = perms[torch.argmin(cost, dim=1)]                            # (B, ntip)
    return torch.gather(targets, 1, best[:, :, None].expand(-1, -1, 3)), (low[:, 1] - low[:, 0]).numpy()


def fit_steps(kin, order, R0, p0, targets, normals, steps, theta0=None):
    """the fit after each step count of `steps` (ascending): a list of dicts
    rot (B, 3, 3), pos, joints, loss (the loss the last step started from; 0
    without a step), gap (steps + 1, B: the assignment gap of the initial
    assignment, then of every step) and on_bound (B, ndof).  order: the chosen
    contact point of every tip, (ntip,) or per candidate (B, ntip); theta0: the
    initial joints when not the model's pre-grasp."""
    R0 = np.asarray(R0, np.float64).reshape(-1, 3, 3)
    B, nt, nd = len(R0), len(kin.fingertip_idx), kin.num_dofs
    order = np.broadcast_to(np.asarray(order, np.int64), (B, nt))
    tipP = torch.tensor(kin.tip_contacts[np.arange(nt)[None, :], order], dtype=torch.float64)      # (B, nt, 3)
    tipN = torch.tensor(kin.tip_normals, dtype=torch.float64).expand(B, nt, 3)
    Tt = torch.tensor(np.asarray(targets, np.float64).reshape(B, nt, 3))
    Nt = torch.tensor(np.asarray(normals, np.float64).reshape(B, nt, 3))
    perms = torch.tensor(list(permutations(range(nt))), dtype=torch.int64)
    th0 = np.broadcast_to(kin.pregrasp if theta0 is None else np.asarray(theta0, np.float64), (B, nd)).copy()
    lo, hi = kin.joint_ranges[:, 0], kin.joint_ranges[:, 1]

    def world(R, p, frames, pts):
        x = _qapply(frames[..., :4], pts) + frames[..., 4:]
        return torch.einsum("bij,bnj->bni", R, x) + p[:, None, :]

    with torch.no_grad():
        fr = _tip_frames(kin, torch.tensor(th0))
        tip0 = world(torch.tensor(R0), torch.tensor(np.asarray(p0, np.float64).reshape(B, 3)), fr, tipP)
        assigned, gap0 = _assign(tip0, Tt, perms)
    gaps = [gap0]
    prm = np.concatenate([R0[:, :2, :].reshape(B, 6), np.asarray(p0, np.float64).reshape(B, 3), th0], axis=1)
    m, v = np.zeros_like(prm), np.zeros_like(prm)
    loss = np.zeros(B)
    out = []

    def snapshot():
        with torch.no_grad():
            rot = _rot6(torch.tensor(prm[:, :6])).numpy()
        return dict(rot=rot, pos=prm[:, 6:9].copy(), joints=prm[:, 9:].copy(), loss=loss.copy(),
                    gap=np.array(gaps), on_bound=(prm[:, 9:] == lo) | (prm[:, 9:] == hi))

    steps = list(steps)
    if steps and steps[0] == 0:
        out.append(snapshot())
    for it in range(1, (max(steps) if steps else 0) + 1):
        x = torch.tensor(prm, requires_grad=True)
        R = _rot6(x[:, :6])
        fr = _tip_frames(kin, x[:, 9:])
        pos = world(R, x[:, 6:9], fr, tipP)
        origin = world(R, x[:, 6:9], fr, torch.zeros_like(tipP))
        npoint = world(R, x[:, 6:9], fr, tipN)
        cos = (Nt * (npoint - origin)).sum(-1)
        with torch.no_grad():
            tgt, gap = _assign(pos, assigned, perms)
        each = ((tgt - pos) ** 2).mean(dim=(1, 2)) + COS_WEIGHT * (0.5 * (1.0 - cos)).mean(dim=1)
        each.sum().backward()
        g = x.grad.numpy()
        loss = each.detach().numpy().copy()
        gaps.append(gap)
        # optax.adamw: scale_by_adam -> add_decayed_weights -> scale(-lr); then the clip
        m = (1.0 - B1) * g + B1 * m
        v = (1.0 - B2) * (g * g) + B2 * v
        upd = (m / (1.0 - B1 ** it)) / (np.sqrt(v / (1.0 - B2 ** it)) + ADAM_EPS) + WEIGHT_DECAY * prm
        prm = prm - LR * upd
        prm[:, 9:] = np.clip(prm[:, 9:], lo, hi)
        if it in steps:
            out.append(snapshot())
    return out


def fit(kin, order, R0, p0, targets, normals, iters, theta0=None):
    """the fit after `iters` steps: see fit_steps"""
    return fit_steps(kin, order, R0, p0, targets, normals, [iters], theta0)[0]


def fit_case(kin, n=6, seed=7):
    """(R0, p0, targets, normals) of n candidates: a random rotation times the
    model's approach alignment, positions and targets a few centimetres out"""
    rng = np.random.default_rng(seed)
    R = np.einsum("nij,jk->nik", np.linalg.qr(rng.normal(size=(n, 3, 3)))[0], kin.align_rot)
    p = rng.normal(size=(n, 3)) * 0.05
    Tg = rng.normal(size=(n, 5, 3)) * 0.04
    N = rng.normal(size=(n, 5, 3))
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    return R, p, Tg, N


FIT_ORDERS = ([2, 1, 0, 1, 2], [0, 1, 2, 0, 1])
FIT_STEPS = (1, 5, 20)


def one_ulp(a, rng):
    """every entry moved by one unit in the last place, up or down at random"""
    a = np.asarray(a, np.float64)
    return a + np.where(rng.random(a.shape) < 0.5, -1.0, 1.0) * np.spacing(np.abs(a))


@lru_cache(maxsize=None)
def fit_reference():
    """the shared fit truth of the CPU and GPU tests: both orders of the six
    candidates after 0, 1, 5 and 20 steps, and the same from inputs moved by one
    ulp (the truth's own sensitivity).  One batched run of 24 candidates.
    Returns (kin, case, {order index: [result per step count]}, {steps: sensitivity})."""
    from mgs.sampler.kin.model import ShadowKinematicsModel
    kin = ShadowKinematicsModel()
    R, p, Tg, N = fit_case(kin)
    n = len(R)
    rng = np.random.default_rng(8)
    Rq, pq, thq = one_ulp(R, rng), one_ulp(p, rng), one_ulp(np.tile(kin.pregrasp, (n, 1)), rng)
    th = np.tile(kin.pregrasp, (n, 1))
    order = np.concatenate([np.tile(o, (2 * n, 1)) for o in FIT_ORDERS])
    steps = (0,) + FIT_STEPS
    res = fit_steps(kin, order, np.concatenate([R, Rq] * 2), np.concatenate([p, pq] * 2), np.concatenate([Tg] * 4),
                    np.concatenate([N] * 4), steps, theta0=np.concatenate([th, thq] * 2))

    def part(r, a):
        return {k: (v[:, a:a + n] if k == "gap" else v[a:a + n]) for k, v in r.items()}
    base = {q: [part(r, 2 * n * q) for r in res] for q in range(len(FIT_ORDERS))}
    moved = {q: [part(r, 2 * n * q + n) for r in res] for q in range(len(FIT_ORDERS))}
    sens = {}
    for s, it in enumerate(steps):
        sens[it] = max(float(np.abs(base[q][s][k] - moved[q][s][k]).max())
                       for q in base for k in ("rot", "pos", "joints", "loss"))
    return kin, (R, p, Tg, N), base, sens


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def check_fit(run, kin_desc, reference):
    """the comparison the CPU test makes of the oracle and the GPU test of the
    kernel: run(desc, R, p, T, N) -> dict of rot, pos, joints, loss, with desc =
    kin_desc(kin, order, iters=...), against fit_reference() within 64 times its
    sensitivity; a candidate whose assignment gap drops below 1e-6 is left out
    (one at the most); some joint ends on a range bound"""
    kin, (R, p, Tg, N), base, sens = reference
    on_bound = False
    for q, order in enumerate(FIT_ORDERS):
        gap = base[q][-1]["gap"].min(axis=0)                 # per candidate, over the 20 steps
        keep = gap >= 1e-6
        assert np.count_nonzero(~keep) <= 1
        for s, it in enumerate((0,) + FIT_STEPS):
            if it == 0:
                continue
            bound = 64 * sens[it]
            print(f"order {order} steps {it}: sensitivity {sens[it]:.3g}, bound {bound:.3g}, smallest gap "
                  f"{gap.min():.3g}, left out {np.count_nonzero(~keep)}")
            assert bound < 1e-12
            got = run(kin_desc(kin, order, iters=it), R, p, Tg, N)
            for k in ("rot", "pos", "joints", "loss"):
                err = np.abs(got[k][keep] - base[q][s][k][keep]).max()
                print(f"    {k}: {err:.3g}")
                assert err <= bound, (order, it, k)
            on_bound = on_bound or bool(base[q][s]["on_bound"][keep].any())
    assert on_bound                                          # the clip is exercised


def check_fit_zero_steps(run, kin_desc, reference):
    """without a step: the pre-grasp joints bit for bit (the first knuckle below
    its range included), loss 0, the position untouched, rot the Gram-Schmidt
    matrix of the first two rows of R0"""
    kin, (R, p, Tg, N), base, _ = reference
    for q, order in enumerate(FIT_ORDERS):
        got = run(kin_desc(kin, order, iters=0), R, p, Tg, N)
        want = base[q][0]
        assert np.array_equal(_bits(got["joints"]), _bits(np.tile(kin.pregrasp, (len(R), 1))))
        assert got["joints"][0, 0] < kin.joint_ranges[0, 0]              # the knuckle below its range, unclipped
        assert np.array_equal(_bits(got["loss"]), np.zeros(len(R), np.int64))
        assert np.array_equal(_bits(got["pos"]), _bits(p))
        # Gram-Schmidt of the first two rows of R0: a dozen roundings of values below 1
        assert np.abs(got["rot"] - want["rot"]).max() <= 8 * np.finfo(float).eps
        b1 = R[:, 0] / np.linalg.norm(R[:, 0], axis=1, keepdims=True)
        b2 = R[:, 1] - np.sum(b1 * R[:, 1], axis=1, keepdims=True) * b1
        b2 /= np.linalg.norm(b2, axis=1, keepdims=True)
        assert np.abs(got["rot"] - np.stack([b1, b2, np.cross(b1, b2)], axis=1)).max() <= 8 * np.finfo(float).eps
