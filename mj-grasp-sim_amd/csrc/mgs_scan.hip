// mgs_scan.hip -- depth / segmentation ray casting of a clutter scene and the
// point-cloud step behind it on the MI355X (reference: MjScanEnv.scan,
// mgs/env/base.py:77-126, and rgbd_to_pcd, mgs/util/img_proc.py:38-62; the
// reference renders with OpenGL, this build casts one ray per pixel).
//
// mgs_scan_kernel: one lane per pixel, a workgroup per 16 x 16 pixel tile and a
// wave per 8 x 8 block of it, so the rays of a wave walk the same nodes.  The
// drawable headers (type, id, mesh, pose, size) are staged through LDS in
// groups of MGS_SCAN_STAGE.  A mesh instance rotates the ray into the mesh
// frame (rigid: t is unchanged) and walks the mesh's threaded BVH: nodes in
// depth-first order, node i + 1 is the first child, skip[i] the node after the
// subtree, so the walk keeps no stack and has one order.  The nearest hit is
// the lexicographic minimum of (t, drawable index, original face id), which
// does not depend on that order; ntest counts the ray-triangle tests, which
// does.  Triangles go through ray_tri (mgs_sampler.hip); all arithmetic is f64
// without contraction, expression for expression what tests/scan_truth.py
// restates in numpy.  Capsules and capped cylinders (a gripper's collision
// geometry, GripperScanEnv) go through scan_rod in the geom frame the box
// branch uses; tests/gripper_scan_truth.py restates it.
//
// mgs_scan_points_kernel: one lane per pixel: the valid mask (seg != -1) eroded
// erode_iters times by a 3 x 3 square with the outside counted as set -- the
// AND over the (2 iters + 1)^2 window clipped to the image --, the reference's
// back-projection (no half-pixel offset), the 4 x 4 extrinsic and the region box.

#define MGS_SCAN_TILE 16
#define MGS_SCAN_STAGE 32
#define MGS_SCAN_HDR 15   // doubles per staged drawable: pos 3, rot 9, size 3

struct ScanDev {
  int ndraw;
  const int32_t *dtype, *did, *dmesh;
  const double *dpos, *drot, *dsize;
  const int32_t *mnode0, *mtri0;
  const double* nbox;
  const int32_t *nskip, *nfirst, *ncount;
  const double* tri;
  const int32_t* face;
};

// slab test of the ray o + t d against the box [lo, hi]; inv = 1 / d.  A zero
// direction component is an inside test of that axis.  Returns whether the line
// meets the box, with the entry and exit parameters.
DEVI int scan_slab(const double* o, const double* d, const double* inv, const double* lo, const double* hi,
                   double* tn, double* tf) {
  double tnear = -INFINITY, tfar = INFINITY;
  for (int k = 0; k < 3; k++) {
    if (d[k] == 0.0) {
      if (o[k] < lo[k] || o[k] > hi[k]) return 0;
    } else {
      double a = (lo[k] - o[k]) * inv[k], b = (hi[k] - o[k]) * inv[k];
      double mn = a < b ? a : b, mx = a < b ? b : a;
      if (mn > tnear) tnear = mn;
      if (mx < tfar) tfar = mx;
    }
  }
  *tn = tnear;
  *tf = tfar;
  return tnear <= tfar;
}

// the ray om + t dm (geom frame) against a rod of radius r and half-length h
// about the frame's z: a capped cylinder (cyl != 0) or a capsule.  Returns the
// smallest t > 0 over the pieces -- from inside that is the exit -- or INFINITY.
//   side  (dm0^2 + dm1^2) t^2 + 2 (om0 dm0 + om1 dm1) t + (om0^2 + om1^2 - r^2) = 0,
//         a root counts where |om2 + t dm2| <= h; no side test if dm0^2 + dm1^2 == 0
//   caps  t = (+-h - om2) / dm2, counts where x^2 + y^2 <= r^2; none if dm2 == 0
//   ends  the spheres about (0, 0, +-h), each root only on its outer half,
//         +-(z -+ h) >= 0
// cyl is the same for every lane of a wave (one drawable at a time).
DEVI double scan_rod(const double* om, const double* dm, double r, double h, int cyl) {
  double t = INFINITY;
  const double rr = r * r;
  const double a = dm[0] * dm[0] + dm[1] * dm[1];
  if (a > 0.0) {
    double b = om[0] * dm[0] + om[1] * dm[1];
    double c = (om[0] * om[0] + om[1] * om[1]) - rr;
    double disc = b * b - a * c;
    if (disc >= 0.0) {
      double s = sqrt(disc);
      double t0 = (-b - s) / a, t1 = (-b + s) / a;
      if (t0 > 0.0 && fabs(om[2] + t0 * dm[2]) <= h && t0 < t) t = t0;
      if (t1 > 0.0 && fabs(om[2] + t1 * dm[2]) <= h && t1 < t) t = t1;
    }
  }
  if (cyl) {
    if (dm[2] != 0.0) {
      for (int e = 0; e < 2; e++) {
        double tc = ((e ? -h : h) - om[2]) / dm[2];
        double x = om[0] + tc * dm[0], y = om[1] + tc * dm[1];
        if (tc > 0.0 && (x * x + y * y) <= rr && tc < t) t = tc;
      }
    }
    return t;
  }
  const double A = a + dm[2] * dm[2];
  for (int e = 0; e < 2; e++) {
    const double sg = e ? -1.0 : 1.0;
    double w = om[2] - sg * h;
    double B = (om[0] * dm[0] + om[1] * dm[1]) + w * dm[2];
    double C = ((om[0] * om[0] + om[1] * om[1]) + w * w) - rr;
    double disc = B * B - A * C;
    if (disc >= 0.0) {
      double s = sqrt(disc);
      double t0 = (-B - s) / A, t1 = (-B + s) / A;
      if (t0 > 0.0 && sg * (w + t0 * dm[2]) >= 0.0 && t0 < t) t = t0;
      if (t1 > 0.0 && sg * (w + t1 * dm[2]) >= 0.0 && t1 < t) t = t1;
    }
  }
  return t;
}

__global__ void __launch_bounds__(MGS_SCAN_TILE * MGS_SCAN_TILE)
mgs_scan_kernel(ScanDev S, const double* __restrict__ cam_pos, const double* __restrict__ cam_rot, int width,
                int height, double fx, double fy, double cx, double cy, double* __restrict__ out_depth,
                int32_t* __restrict__ out_seg, int32_t* __restrict__ out_tri, int32_t* __restrict__ out_ntest) {
  __shared__ double s_hdr[MGS_SCAN_STAGE * MGS_SCAN_HDR];
  __shared__ int32_t s_int[MGS_SCAN_STAGE * 3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = blockIdx.x * MGS_SCAN_TILE + (wave & 1) * 8 + (lane & 7);
  const int row = blockIdx.y * MGS_SCAN_TILE + (wave >> 1) * 8 + (lane >> 3);
  const int view = blockIdx.z;
  const bool act = col < width && row < height;
  double o[3], d[3];
  {
    const double* R = cam_rot + 9 * (size_t)view;
    double dc0 = (((double)col + 0.5) - cx) / fx, dc1 = (((double)row + 0.5) - cy) / fy;
    for (int k = 0; k < 3; k++) {
      o[k] = cam_pos[3 * (size_t)view + k];
      d[k] = (R[3 * k] * dc0 + R[3 * k + 1] * dc1) + R[3 * k + 2];
    }
  }
  double best_t = INFINITY;
  int best_draw = -1, best_seg = -1, best_face = -1, ntest = 0;
  for (int base = 0; base < S.ndraw; base += MGS_SCAN_STAGE) {
    const int m = S.ndraw - base < MGS_SCAN_STAGE ? S.ndraw - base : MGS_SCAN_STAGE;
    __syncthreads();
    for (int k = tid; k < m * MGS_SCAN_HDR; k += blockDim.x) {
      int j = k / MGS_SCAN_HDR, e = k - j * MGS_SCAN_HDR;
      size_t g = (size_t)(base + j);
      s_hdr[k] = e < 3 ? S.dpos[3 * g + e] : e < 12 ? S.drot[9 * g + (e - 3)] : S.dsize[3 * g + (e - 12)];
    }
    for (int k = tid; k < m; k += blockDim.x) {
      s_int[3 * k] = S.dtype[base + k];
      s_int[3 * k + 1] = S.did[base + k];
      s_int[3 * k + 2] = S.dmesh[base + k];
    }
    __syncthreads();
    if (!act) continue;
    for (int j = 0; j < m; j++) {
      const double* pos = s_hdr + j * MGS_SCAN_HDR;
      const double* R = pos + 3;
      const double* size = pos + 12;
      const int type = s_int[3 * j], di = base + j;
      double v[3];
      for (int k = 0; k < 3; k++) v[k] = o[k] - pos[k];
      if (type == MGS_SCAN_SPHERE) {
        double a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        double b = (v[0] * d[0] + v[1] * d[1]) + v[2] * d[2];
        double c = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) - size[0] * size[0];
        double disc = b * b - a * c;
        if (disc >= 0.0) {
          double s = sqrt(disc);
          double t0 = (-b - s) / a, t1 = (-b + s) / a;
          double t = t0 > 0.0 ? t0 : t1;
          if (t > 0.0 && t < best_t) { best_t = t; best_draw = di; best_seg = s_int[3 * j + 1]; best_face = -1; }
        }
        continue;
      }
      // the ray in the geom frame: R^T (o - pos), R^T d
      double om[3], dm[3], inv[3];
      for (int k = 0; k < 3; k++) {
        om[k] = (R[k] * v[0] + R[3 + k] * v[1]) + R[6 + k] * v[2];
        dm[k] = (R[k] * d[0] + R[3 + k] * d[1]) + R[6 + k] * d[2];
        inv[k] = 1.0 / dm[k];
      }
      if (type == MGS_SCAN_BOX) {
        double lo[3] = {-size[0], -size[1], -size[2]}, tn, tf;
        if (scan_slab(om, dm, inv, lo, size, &tn, &tf)) {
          double t = tn > 0.0 ? tn : tf;     // from inside: the exit
          if (t > 0.0 && t < best_t) { best_t = t; best_draw = di; best_seg = s_int[3 * j + 1]; best_face = -1; }
        }
        continue;
      }
      if (type == MGS_SCAN_CAPSULE || type == MGS_SCAN_CYLINDER) {
        double t = scan_rod(om, dm, size[0], size[1], type == MGS_SCAN_CYLINDER);
        if (t < best_t) { best_t = t; best_draw = di; best_seg = s_int[3 * j + 1]; best_face = -1; }
        continue;
      }
      const int mesh = s_int[3 * j + 2];
      const int node0 = S.mnode0[mesh], nnode = S.mnode0[mesh + 1] - node0, tri0 = S.mtri0[mesh];
      int i = 0;
      while (i < nnode) {
        const int g = node0 + i;
        const double* box = S.nbox + 6 * (size_t)g;
        double lo[3] = {box[0], box[1], box[2]}, hi[3] = {box[3], box[4], box[5]}, tn, tf;
        if (scan_slab(om, dm, inv, lo, hi, &tn, &tf) && tf >= 0.0 && tn <= best_t) {
          const int cnt = S.ncount[g];
          if (cnt == 0) { i = i + 1; continue; }
          const int first = tri0 + S.nfirst[g];
          for (int q = 0; q < cnt; q++) {
            double t;
            ntest++;
            if (ray_tri(om, dm, S.tri + 9 * (size_t)(first + q), &t)) {
              const int f = S.face[first + q];
              if (t < best_t || (t == best_t && best_draw == di && f < best_face)) {
                best_t = t; best_draw = di; best_seg = s_int[3 * j + 1]; best_face = f;
              }
            }
          }
        }
        i = S.nskip[g];
      }
    }
  }
  if (act) {
    size_t p = ((size_t)view * height + row) * width + col;
    out_depth[p] = best_draw >= 0 ? best_t : 0.0;
    out_seg[p] = best_seg;
    out_tri[p] = best_face;
    out_ntest[p] = ntest;
  }
}

__global__ void __launch_bounds__(256)
mgs_scan_points_kernel(int nview, int width, int height, const double* __restrict__ depth,
                       const int32_t* __restrict__ seg, const double* __restrict__ extr, double fx, double fy,
                       double cx, double cy, int iters, double lo0, double lo1, double lo2, double hi0, double hi1,
                       double hi2, double* __restrict__ out_points, uint8_t* __restrict__ out_keep) {
  const size_t npix = (size_t)width * height, n = npix * nview;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int view = (int)(p / npix);
  const int r = (int)((p - view * npix) / width), c = (int)(p - view * npix - (size_t)r * width);
  int ok = 1;
  const int r0 = r - iters < 0 ? 0 : r - iters, r1 = r + iters > height - 1 ? height - 1 : r + iters;
  const int c0 = c - iters < 0 ? 0 : c - iters, c1 = c + iters > width - 1 ? width - 1 : c + iters;
  const int32_t* sv = seg + view * npix;
  for (int rr = r0; rr <= r1 && ok; rr++)
    for (int cc = c0; cc <= c1; cc++)
      if (sv[(size_t)rr * width + cc] == -1) { ok = 0; break; }
  const double z = depth[p];
  const double x = (((double)c - cx) * z) / fx, y = (((double)r - cy) * z) / fy;
  const double* E = extr + 16 * (size_t)view;
  double q[3];
  for (int k = 0; k < 3; k++) q[k] = ((E[4 * k] * x + E[4 * k + 1] * y) + E[4 * k + 2] * z) + E[4 * k + 3];
  for (int k = 0; k < 3; k++) out_points[3 * p + k] = q[k];
  out_keep[p] = ok && q[0] > lo0 && q[0] < hi0 && q[1] > lo1 && q[1] < hi1 && q[2] > lo2 && q[2] < hi2;
}
