// mgs_aux.hip -- the library's non-template kernels: the capacity escalation's
// overflow list and the device-side probes of the tests.  Included by
// mgs_capi.hip only (after mgs_kernels.hip).

// capacity-escalation list: indices of the candidates whose stats flags meet
// mask (order of arrival; each re-run is independent of the order)
__global__ void __launch_bounds__(256)
mgs_overflow_list_kernel(const int32_t* __restrict__ stats, int n, int mask, int32_t* __restrict__ count,
                         int32_t* __restrict__ list) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (stats[MGS_NSTATS * i + 2] & mask)) list[atomicAdd(count, 1)] = i;
}

// device-side arithmetic probe (tests): sqrt, division, sincos against the oracle
extern "C" __global__ void mgs_arith_probe_kernel(const double* x, const double* y, int n, double* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s, c;
  k_sincos(x[i], &s, &c);
  out[4 * i] = sqrt(fabs(x[i]));
  out[4 * i + 1] = x[i] / y[i];
  out[4 * i + 2] = s;
  out[4 * i + 3] = c;
}

// tree-reduction probe (tests): out[b] = tree_sum over lanes of a[b*64+l]*c[b*64+l] with P = nextpow2(n)
extern "C" __global__ void __launch_bounds__(64) mgs_tree_probe_kernel(const double* a, const double* c, int n,
                                                                         double* out) {
  int l = lane_id();
  int b = blockIdx.x;
  double leaf = (l < n) ? a[b * 64 + l] * c[b * 64 + l] : 0.0;
  double s = tree_sum(leaf, next_pow2(n));
  if (l == 0) out[b] = s;
}
