// mgs_cloud.hip -- the scene cloud behind the scan on the MI355X: stable
// compaction of the kept pixels, the 2 mm voxel grid of
// mgs.util.img_proc.voxel_downsample_pcd and an exact, spatially pruned
// farthest-point pick (include/mgs_gpu.h "Scene cloud").  Included
// from mgs_capi.hip only.  f64 without contraction; tests/cloud_truth.py
// restates every stage in numpy in the same order of operations.
//
// No workgroup waits on another: every prefix sum is three launches (block
// sums, one workgroup scanning the block sums, blocks rescanning with their
// offset), and the pick is one workgroup.  Atomics are integer adds whose
// arrival order changes no result: the per-cell counts, and the slot a point
// takes inside its cell, which the voxel stage sorts back into ascending index
// and the pick never looks at (its maxima break ties by the original index).
//
// Voxel stage (cells of the dense grid in ascending raveled (x, y, z) order):
//   cloud_flag_kernel      per block of 2048 inputs: kept count, min / max of
//                          the kept points, a non-finite flag
//   cloud_scan_sums_kernel one workgroup: exclusive scan of the block sums,
//                          the total, and the min / max / flag reduced
//   cloud_compact_kernel   kept inputs to their rank: point, features (given,
//                          or the colour-table row of the segmentation id),
//                          cell by numpy's floor_divide rule, count grid += 1
//   cloud_cell_sums_kernel / cloud_cell_offsets_kernel
//                          (occupied, count) scanned over the cells: the rank of
//                          an occupied cell is its voxel, its offset the first
//                          slot; the grid then holds each cell's next free slot
//   cloud_scatter_kernel   point -> a slot of its cell
//   cloud_voxel_kernel     one lane per voxel: slots into ascending index, then
//                          the sums in np.add.at order and the means
// Pick stage (buckets = occupied cells of a coarse grid, same machinery):
//   cloud_fps_cell_kernel  cell = floor((p - min) / side) per axis
//   cloud_fps_gather_kernel, cloud_fps_box_kernel
//                          bucket-contiguous points, boxes, maxima = +inf
//   mgs_cloud_fps_kernel   one workgroup of 1024 lanes, per pick: lanes over
//                          buckets test lb < max and list the buckets to visit
//                          in LDS; a wave per listed bucket updates its points'
//                          running minima and the bucket's (max, lowest index);
//                          all lanes reduce the bucket table to the next pick.
//   mgs_cloud_fps_batch_kernel
//                          the same loop (cloud_fps_pick), one workgroup per
//                          cloud of a job table: many clouds' picks at once.

#define MGS_CLOUD_BLOCK 256
#define MGS_CLOUD_ITEMS 8
#define MGS_CLOUD_CHUNK (MGS_CLOUD_BLOCK * MGS_CLOUD_ITEMS)
#define MGS_CLOUD_FPS_THREADS 1024
#define MGS_CLOUD_FPS_TILE 4096      // buckets tested per pass: the LDS visit list

typedef unsigned long long cloud_u64;

// header the scan of the block sums leaves: total, min xyz, max xyz, flag
struct CloudHdr {
  cloud_u64 total;
  double lo[3], hi[3];
  int32_t bad, pad;
};

// numpy's float floor_divide for a >= 0, b > 0 (npy_divmod)
__host__ __device__ inline double cloud_floor_divide(double a, double b) {
  double mod = fmod(a, b);
  double div = (a - mod) / b;
  if (div == 0.0) return 0.0;
  double f = floor(div);
  if (div - f > 0.5) f += 1.0;
  return f;
}

// exclusive scan of v over the 256 lanes of a block in lane order; *total = the
// block's sum.  s_w: 4 words of LDS.  Two barriers.
DEVI cloud_u64 cloud_block_scan(cloud_u64 v, cloud_u64* s_w, cloud_u64* total) {
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  cloud_u64 inc = v;
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) {
    cloud_u64 o = __shfl_up(inc, s);
    if (lane >= s) inc += o;
  }
  __syncthreads();
  if (lane == WAVE - 1) s_w[w] = inc;
  __syncthreads();
  cloud_u64 before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < MGS_CLOUD_BLOCK / WAVE; q++) {
    cloud_u64 x = s_w[q];
    if (q < w) before += x;
    all += x;
  }
  *total = all;
  return before + (inc - v);
}

DEVI cloud_u64 cloud_block_sum(cloud_u64 v, cloud_u64* s_w) {
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) v += __shfl_xor(v, s);
  __syncthreads();
  if (lane == 0) s_w[w] = v;
  __syncthreads();
  cloud_u64 all = 0;
#pragma unroll
  for (int q = 0; q < MGS_CLOUD_BLOCK / WAVE; q++) all += s_w[q];
  return all;
}

__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_flag_kernel(const double* __restrict__ x, const uint8_t* __restrict__ keep, size_t n,
                  cloud_u64* __restrict__ sums, double* __restrict__ blo, double* __restrict__ bhi,
                  int32_t* __restrict__ bbad) {
  __shared__ cloud_u64 s_w[MGS_CLOUD_BLOCK / WAVE];
  __shared__ double s_lo[MGS_CLOUD_BLOCK / WAVE][3], s_hi[MGS_CLOUD_BLOCK / WAVE][3];
  __shared__ int s_bad[MGS_CLOUD_BLOCK / WAVE];
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  const size_t base = (size_t)blockIdx.x * MGS_CLOUD_CHUNK;
  cloud_u64 cnt = 0;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  for (int i = 0; i < MGS_CLOUD_ITEMS; i++) {
    const size_t j = base + (size_t)i * MGS_CLOUD_BLOCK + t;
    if (j >= n || (keep && !keep[j])) continue;
    cnt++;
    for (int k = 0; k < 3; k++) {
      const double v = x[3 * j + k];
      if (!(fabs(v) <= 1.7976931348623157e308)) bad = 1;      // inf or nan
      if (v < lo[k]) lo[k] = v;
      if (v > hi[k]) hi[k] = v;
    }
  }
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) {
    for (int k = 0; k < 3; k++) {
      double a = __shfl_xor(lo[k], s), b = __shfl_xor(hi[k], s);
      if (a < lo[k]) lo[k] = a;
      if (b > hi[k]) hi[k] = b;
    }
    bad |= __shfl_xor(bad, s);
  }
  if (lane == 0) {
    for (int k = 0; k < 3; k++) { s_lo[w][k] = lo[k]; s_hi[w][k] = hi[k]; }
    s_bad[w] = bad;
  }
  const cloud_u64 all = cloud_block_sum(cnt, s_w);      // its barriers also publish s_lo / s_hi / s_bad
  if (t == 0) {
    for (int q = 1; q < MGS_CLOUD_BLOCK / WAVE; q++) {
      for (int k = 0; k < 3; k++) {
        if (s_lo[q][k] < lo[k]) lo[k] = s_lo[q][k];
        if (s_hi[q][k] > hi[k]) hi[k] = s_hi[q][k];
      }
      bad |= s_bad[q];
    }
    sums[blockIdx.x] = all;
    for (int k = 0; k < 3; k++) { blo[3 * (size_t)blockIdx.x + k] = lo[k]; bhi[3 * (size_t)blockIdx.x + k] = hi[k]; }
    bbad[blockIdx.x] = bad;
  }
}

// one workgroup: sums[0 .. nb) -> their exclusive scan, hdr->total = the sum;
// with blo: the min / max / flag of the blocks into hdr
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_scan_sums_kernel(cloud_u64* __restrict__ sums, size_t nb, const double* __restrict__ blo,
                       const double* __restrict__ bhi, const int32_t* __restrict__ bbad, CloudHdr* __restrict__ hdr) {
  __shared__ cloud_u64 s_w[MGS_CLOUD_BLOCK / WAVE];
  __shared__ double s_lo[MGS_CLOUD_BLOCK / WAVE][3], s_hi[MGS_CLOUD_BLOCK / WAVE][3];
  __shared__ int s_bad[MGS_CLOUD_BLOCK / WAVE];
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  cloud_u64 carry = 0;
  for (size_t base = 0; base < nb; base += MGS_CLOUD_BLOCK) {
    const size_t j = base + t;
    const cloud_u64 v = j < nb ? sums[j] : 0;
    cloud_u64 all;
    const cloud_u64 ex = cloud_block_scan(v, s_w, &all);
    if (j < nb) sums[j] = carry + ex;
    carry += all;
  }
  if (t == 0) hdr->total = carry;
  if (!blo) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  for (size_t j = t; j < nb; j += MGS_CLOUD_BLOCK) {
    for (int k = 0; k < 3; k++) {
      const double a = blo[3 * j + k], b = bhi[3 * j + k];
      if (a < lo[k]) lo[k] = a;
      if (b > hi[k]) hi[k] = b;
    }
    bad |= bbad[j];
  }
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) {
    for (int k = 0; k < 3; k++) {
      double a = __shfl_xor(lo[k], s), b = __shfl_xor(hi[k], s);
      if (a < lo[k]) lo[k] = a;
      if (b > hi[k]) hi[k] = b;
    }
    bad |= __shfl_xor(bad, s);
  }
  __syncthreads();
  if (lane == 0) {
    for (int k = 0; k < 3; k++) { s_lo[w][k] = lo[k]; s_hi[w][k] = hi[k]; }
    s_bad[w] = bad;
  }
  __syncthreads();
  if (t == 0) {
    for (int q = 1; q < MGS_CLOUD_BLOCK / WAVE; q++) {
      for (int k = 0; k < 3; k++) {
        if (s_lo[q][k] < lo[k]) lo[k] = s_lo[q][k];
        if (s_hi[q][k] > hi[k]) hi[k] = s_hi[q][k];
      }
      bad |= s_bad[q];
    }
    for (int k = 0; k < 3; k++) { hdr->lo[k] = lo[k]; hdr->hi[k] = hi[k]; }
    hdr->bad = bad;
  }
}

struct CloudGrid {
  double lo[3];
  double side;
  int64_t dim[3];
};

DEVI uint32_t cloud_voxel_cell(const CloudGrid& G, const double* p) {
  int64_t c[3];
  for (int k = 0; k < 3; k++) {
    double f = cloud_floor_divide(p[k] - G.lo[k], G.side);
    int64_t q = f >= 0.0 ? (f < (double)G.dim[k] ? (int64_t)f : G.dim[k] - 1) : 0;     // in range by monotonicity; held
    c[k] = q;
  }
  return (uint32_t)((c[0] * G.dim[1] + c[1]) * G.dim[2] + c[2]);
}

// kept input j -> rank r (ascending j): cpts[r], cfeat[r], pcell[r]; grid[cell] += 1.
// Features: feat (n * nfeat), or with seg the row seg[j] of colors (ncolor * 3, nfeat 3).
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_compact_kernel(const double* __restrict__ x, const uint8_t* __restrict__ keep, size_t n,
                     const cloud_u64* __restrict__ sums, const float* __restrict__ feat, int nfeat,
                     const int32_t* __restrict__ seg, const float* __restrict__ colors, int ncolor, CloudGrid G,
                     double* __restrict__ cpts, float* __restrict__ cfeat, uint32_t* __restrict__ pcell,
                     uint32_t* __restrict__ grid) {
  __shared__ cloud_u64 s_w[MGS_CLOUD_BLOCK / WAVE];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * MGS_CLOUD_CHUNK;
  cloud_u64 carry = sums[blockIdx.x];
  for (int i = 0; i < MGS_CLOUD_ITEMS; i++) {
    const size_t j = base + (size_t)i * MGS_CLOUD_BLOCK + t;
    const bool k_ = j < n && (!keep || keep[j]);
    cloud_u64 all;
    const cloud_u64 r = carry + cloud_block_scan(k_ ? 1 : 0, s_w, &all);
    carry += all;
    if (!k_) continue;
    double p[3];
    for (int k = 0; k < 3; k++) { p[k] = x[3 * j + k]; cpts[3 * r + k] = p[k]; }
    if (seg) {
      const int32_t s = seg[j];
      for (int c = 0; c < 3; c++) cfeat[3 * r + c] = s >= 0 && s < ncolor ? colors[3 * (size_t)s + c] : 0.f;
    } else {
      for (int c = 0; c < nfeat; c++) cfeat[(size_t)nfeat * r + c] = feat[(size_t)nfeat * j + c];
    }
    const uint32_t cell = cloud_voxel_cell(G, p);
    pcell[r] = cell;
    atomicAdd(&grid[cell], 1u);
  }
}

// (occupied cells << 32 | points) of each block of 2048 cells
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_cell_sums_kernel(const uint32_t* __restrict__ grid, size_t ncell, cloud_u64* __restrict__ sums) {
  __shared__ cloud_u64 s_w[MGS_CLOUD_BLOCK / WAVE];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * MGS_CLOUD_CHUNK;
  cloud_u64 v = 0;
  for (int i = 0; i < MGS_CLOUD_ITEMS; i++) {
    const size_t c = base + (size_t)i * MGS_CLOUD_BLOCK + t;
    const uint32_t g = c < ncell ? grid[c] : 0;
    if (g) v += ((cloud_u64)1 << 32) | g;
  }
  const cloud_u64 all = cloud_block_sum(v, s_w);
  if (t == 0) sums[blockIdx.x] = all;
}

// occupied cell c of rank v: start[v] = its first slot, grid[c] = the same (the
// scatter's cursor); start[nvox] = npts
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_cell_offsets_kernel(uint32_t* __restrict__ grid, size_t ncell, const cloud_u64* __restrict__ sums,
                          uint32_t* __restrict__ start, uint32_t nvox, uint32_t npts) {
  __shared__ cloud_u64 s_w[MGS_CLOUD_BLOCK / WAVE];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * MGS_CLOUD_CHUNK;
  cloud_u64 carry = sums[blockIdx.x];
  if (blockIdx.x == 0 && t == 0) start[nvox] = npts;
  for (int i = 0; i < MGS_CLOUD_ITEMS; i++) {
    const size_t c = base + (size_t)i * MGS_CLOUD_BLOCK + t;
    const uint32_t g = c < ncell ? grid[c] : 0;
    cloud_u64 all;
    const cloud_u64 ex = carry + cloud_block_scan(g ? (((cloud_u64)1 << 32) | g) : 0, s_w, &all);
    carry += all;
    if (g) {
      const uint32_t v = (uint32_t)(ex >> 32), off = (uint32_t)ex;
      if (v < nvox) start[v] = off;
      grid[c] = off;
    }
  }
}

__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_scatter_kernel(const uint32_t* __restrict__ pcell, uint32_t npts, uint32_t* __restrict__ grid,
                     uint32_t* __restrict__ slot_idx) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= npts) return;
  const uint32_t s = atomicAdd(&grid[pcell[j]], 1u);
  if (s < npts) slot_idx[s] = (uint32_t)j;
}

// one lane per voxel: its slots sorted into ascending point index (insertion
// sort in place), then np.add.at's sums: f64 positions from +0.0, float32
// features from +0.0f, and the means
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_voxel_kernel(const uint32_t* __restrict__ start, uint32_t nvox, uint32_t* __restrict__ slot_idx,
                   const double* __restrict__ cpts, const float* __restrict__ cfeat, int nfeat,
                   double* __restrict__ vpts, float* __restrict__ vfeat, int32_t* __restrict__ vcnt) {
  const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nvox) return;
  const uint32_t s = start[v], e = start[v + 1];
  for (uint32_t i = s + 1; i < e; i++) {
    const uint32_t key = slot_idx[i];
    uint32_t q = i;
    while (q > s && slot_idx[q - 1] > key) { slot_idx[q] = slot_idx[q - 1]; q--; }
    slot_idx[q] = key;
  }
  const double cnt = (double)(e - s);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (uint32_t i = s; i < e; i++) {
    const size_t j = slot_idx[i];
    a0 += cpts[3 * j];
    a1 += cpts[3 * j + 1];
    a2 += cpts[3 * j + 2];
  }
  vpts[3 * v] = a0 / cnt;
  vpts[3 * v + 1] = a1 / cnt;
  vpts[3 * v + 2] = a2 / cnt;
  for (int c = 0; c < nfeat; c++) {
    float f = 0.f;
    for (uint32_t i = s; i < e; i++) f += cfeat[(size_t)nfeat * slot_idx[i] + c];
    vfeat[(size_t)nfeat * v + c] = (float)((double)f / cnt);
  }
  vcnt[v] = (int32_t)(e - s);
}

// ---------------------------------------------------------------------------
// the cloud path's small steps
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_round_f32_kernel(const double* __restrict__ in, size_t n, double* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) out[j] = (double)(float)in[j];
}

// out row i = float32 of voxel idx[i] (or i without idx)
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_gather_kernel(const int32_t* __restrict__ idx, int m, const double* __restrict__ vpts,
                    const float* __restrict__ vfeat, float* __restrict__ out_p, float* __restrict__ out_c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const size_t v = idx ? (size_t)idx[i] : (size_t)i;
  for (int k = 0; k < 3; k++) {
    out_p[3 * (size_t)i + k] = (float)vpts[3 * v + k];
    out_c[3 * (size_t)i + k] = vfeat[3 * v + k];
  }
}

// ---------------------------------------------------------------------------
// farthest-point pick
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_fps_cell_kernel(const double* __restrict__ x, uint32_t n, CloudGrid G, uint32_t* __restrict__ pcell,
                      uint32_t* __restrict__ grid) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int64_t c[3];
  for (int k = 0; k < 3; k++) {
    const double f = floor((x[3 * j + k] - G.lo[k]) / G.side);
    c[k] = f >= 0.0 ? (f < (double)G.dim[k] ? (int64_t)f : G.dim[k] - 1) : 0;      // in range by monotonicity; held
  }
  const uint32_t cell = (uint32_t)((c[0] * G.dim[1] + c[1]) * G.dim[2] + c[2]);
  pcell[j] = cell;
  atomicAdd(&grid[cell], 1u);
}

__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_fps_gather_kernel(const double* __restrict__ x, uint32_t n, const uint32_t* __restrict__ slot_idx,
                        double* __restrict__ bx, double* __restrict__ bdist) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const size_t j = slot_idx[s];
  for (int k = 0; k < 3; k++) bx[3 * s + k] = x[3 * j + k];
  bdist[s] = INFINITY;
}

// one lane per bucket: box of its points, maximum +inf at its lowest index
__global__ void __launch_bounds__(MGS_CLOUD_BLOCK)
cloud_fps_box_kernel(const uint32_t* __restrict__ start, uint32_t nb, const uint32_t* __restrict__ slot_idx,
                     const double* __restrict__ bx, double* __restrict__ bbox, double* __restrict__ bmax,
                     int32_t* __restrict__ bidx) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t first = 0xffffffffu;
  for (uint32_t s = start[b]; s < start[b + 1]; s++) {
    for (int k = 0; k < 3; k++) {
      const double v = bx[3 * (size_t)s + k];
      if (v < lo[k]) lo[k] = v;
      if (v > hi[k]) hi[k] = v;
    }
    if (slot_idx[s] < first) first = slot_idx[s];
  }
  for (int k = 0; k < 3; k++) { bbox[6 * b + k] = lo[k]; bbox[6 * b + 3 + k] = hi[k]; }
  bmax[b] = INFINITY;
  bidx[b] = (int32_t)first;
}

DEVI void cloud_take(double& bv, int& bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// The pick of one cloud by one workgroup (both pick kernels).  x: the points in
// their own order (the pick's coordinates); bx / borig / bdist: bucket-contiguous
// points, their indices, running minima; start (nb + 1), bbox, bmax, bidx: the
// bucket table.  A bucket whose bound lb = |max(lo - p, p - hi, 0)|^2 is >= its
// maximum cannot change (every point's d >= lb by monotone rounding) and is
// skipped.  nevals = distances computed.  The arrays are named as global memory:
// the batched kernel reads their addresses from a table, and a pointer read from
// memory is otherwise a flat one to the compiler (flat loads and stores also
// wait on the LDS counter: 7.0 instead of 6.2 us per pick, measured).
#define CLOUD_G __attribute__((address_space(1)))
DEVI void cloud_fps_pick(const CLOUD_G double* __restrict__ x, const CLOUD_G double* __restrict__ bx,
                         const CLOUD_G uint32_t* __restrict__ borig, CLOUD_G double* __restrict__ bdist,
                         const CLOUD_G uint32_t* __restrict__ start, const CLOUD_G double* __restrict__ bbox,
                         CLOUD_G double* __restrict__ bmax, CLOUD_G int32_t* __restrict__ bidx, int nb, int k,
                         CLOUD_G int32_t* __restrict__ out, CLOUD_G cloud_u64* __restrict__ nevals) {
  __shared__ int s_visit[MGS_CLOUD_FPS_TILE];
  __shared__ int s_nvisit[2];     // alternating per pass: the idle one is reset between the pass's barriers
  __shared__ double wv[MGS_CLOUD_FPS_THREADS / WAVE];
  __shared__ int wi[MGS_CLOUD_FPS_THREADS / WAVE];
  __shared__ cloud_u64 s_ev[MGS_CLOUD_FPS_THREADS / WAVE];
  __shared__ int last;
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  cloud_u64 evals = 0;
  int pass = 0;
  if (t == 0) { last = 0; s_nvisit[0] = 0; s_nvisit[1] = 0; if (k > 0) out[0] = 0; }
  __syncthreads();
  for (int i = 1; i < k; i++) {
    const int li = last;
    const double p0 = x[3 * (size_t)li], p1 = x[3 * (size_t)li + 1], p2 = x[3 * (size_t)li + 2];
    for (int base = 0; base < nb; base += MGS_CLOUD_FPS_TILE) {
      const int top = nb - base < MGS_CLOUD_FPS_TILE ? nb : base + MGS_CLOUD_FPS_TILE;
      for (int b = base + t; b < top; b += MGS_CLOUD_FPS_THREADS) {
        const CLOUD_G double* B = bbox + 6 * (size_t)b;
        double e0 = B[0] - p0, e1 = B[1] - p1, e2 = B[2] - p2;
        const double f0 = p0 - B[3], f1 = p1 - B[4], f2 = p2 - B[5];
        if (f0 > e0) e0 = f0;
        if (f1 > e1) e1 = f1;
        if (f2 > e2) e2 = f2;
        if (!(e0 > 0.0)) e0 = 0.0;
        if (!(e1 > 0.0)) e1 = 0.0;
        if (!(e2 > 0.0)) e2 = 0.0;
        const double lb = (e0 * e0 + e1 * e1) + e2 * e2;
        if (lb < bmax[b]) s_visit[atomicAdd(&s_nvisit[pass], 1)] = b;
      }
      __syncthreads();
      const int nvisit = s_nvisit[pass];
      if (t == 0) s_nvisit[pass ^ 1] = 0;
      pass ^= 1;
      for (int q = w; q < nvisit; q += MGS_CLOUD_FPS_THREADS / WAVE) {
        const int b = s_visit[q];
        const uint32_t s = start[b], e = start[b + 1];
        double bv = -INFINITY;
        int bi = 0x7fffffff;
        for (uint32_t j = s + lane; j < e; j += WAVE) {
          const double d0 = bx[3 * (size_t)j] - p0, d1 = bx[3 * (size_t)j + 1] - p1, d2 = bx[3 * (size_t)j + 2] - p2;
          const double d = (d0 * d0 + d1 * d1) + d2 * d2;
          double c = bdist[j];
          if (d < c) { c = d; bdist[j] = d; }
          cloud_take(bv, bi, c, (int)borig[j]);
        }
#pragma unroll
        for (int sft = 1; sft < WAVE; sft <<= 1) {
          const double ov = __shfl_xor(bv, sft);
          const int oi = __shfl_xor(bi, sft);
          cloud_take(bv, bi, ov, oi);
        }
        if (lane == 0) { bmax[b] = bv; bidx[b] = bi; evals += e - s; }
      }
      __syncthreads();
    }
    // the next pick: the maximum of the bucket maxima, lowest index among equals
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int b = t; b < nb; b += MGS_CLOUD_FPS_THREADS) cloud_take(bv, bi, bmax[b], bidx[b]);
#pragma unroll
    for (int sft = 1; sft < WAVE; sft <<= 1) {
      const double ov = __shfl_xor(bv, sft);
      const int oi = __shfl_xor(bi, sft);
      cloud_take(bv, bi, ov, oi);
    }
    if (lane == 0) { wv[w] = bv; wi[w] = bi; }
    __syncthreads();
    if (t == 0) {
      double v = wv[0];
      int b = wi[0];
      for (int q = 1; q < MGS_CLOUD_FPS_THREADS / WAVE; q++) cloud_take(v, b, wv[q], wi[q]);
      if (b == 0x7fffffff) b = 0;
      out[i] = b;
      last = b;
    }
    __syncthreads();
  }
  if (lane == 0) s_ev[w] = evals;
  __syncthreads();
  if (t == 0) {
    cloud_u64 all = 0;
    for (int q = 0; q < MGS_CLOUD_FPS_THREADS / WAVE; q++) all += s_ev[q];
    *nevals = all;
  }
}

// one cloud: grid 1
__global__ void __launch_bounds__(MGS_CLOUD_FPS_THREADS)
mgs_cloud_fps_kernel(const double* __restrict__ x, const double* __restrict__ bx, const uint32_t* __restrict__ borig,
                     double* __restrict__ bdist, const uint32_t* __restrict__ start, const double* __restrict__ bbox,
                     double* __restrict__ bmax, int32_t* __restrict__ bidx, int nb, int k, int32_t* __restrict__ out,
                     cloud_u64* __restrict__ nevals) {
  cloud_fps_pick((const CLOUD_G double*)x, (const CLOUD_G double*)bx, (const CLOUD_G uint32_t*)borig,
                 (CLOUD_G double*)bdist, (const CLOUD_G uint32_t*)start, (const CLOUD_G double*)bbox,
                 (CLOUD_G double*)bmax, (CLOUD_G int32_t*)bidx, nb, k, (CLOUD_G int32_t*)out, (CLOUD_G cloud_u64*)nevals);
}

// what mgs_cloud_fps_kernel takes, as one record of the batched pick's table
struct CloudFpsJob {
  const double* x;
  const double* bx;
  const uint32_t* borig;
  double* bdist;
  const uint32_t* start;
  const double* bbox;
  double* bmax;
  int32_t* bidx;
  int32_t* out;
  cloud_u64* nevals;
  int32_t nb, k;
};

// many clouds: grid = the jobs, workgroup b picks the cloud of jobs[b] (the host
// puts the heaviest first: workgroups are dispatched in block order).  The
// clouds share nothing, so no workgroup waits on another.  k == 0: nothing is
// written.
__global__ void __launch_bounds__(MGS_CLOUD_FPS_THREADS)
mgs_cloud_fps_batch_kernel(const CloudFpsJob* __restrict__ jobs) {
  const CloudFpsJob J = jobs[blockIdx.x];
  if (J.k <= 0) return;
  cloud_fps_pick((const CLOUD_G double*)J.x, (const CLOUD_G double*)J.bx, (const CLOUD_G uint32_t*)J.borig,
                 (CLOUD_G double*)J.bdist, (const CLOUD_G uint32_t*)J.start, (const CLOUD_G double*)J.bbox,
                 (CLOUD_G double*)J.bmax, (CLOUD_G int32_t*)J.bidx, J.nb, J.k, (CLOUD_G int32_t*)J.out,
                 (CLOUD_G cloud_u64*)J.nevals);
}
