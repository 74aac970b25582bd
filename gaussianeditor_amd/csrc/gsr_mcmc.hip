// gsr_mcmc.hip -- the 3DGS-MCMC strategy (Kheradmand et al. 2024) beside the ADC policy of gsr_densify.hip (DESIGN.md
// section 21): the opacity-gated positional noise of every step, the dead / alive classification with opacity-weighted
// draws, the relocation values and the row scatter of relocation and growth.
//
// Written in torch the noise step is about fifteen elementwise and bmm launches over all P rows and a refine pays nonzero,
// multinomial, bincount and masked assignment with a host synchronisation each.  Here: ONE launch for the noise (no
// workspace, no readback), a handful of launches with ONE readback for the draws, one launch for the values and one per
// role for the scatter.  The draws are integer arithmetic (weights truncated to 23 bits, 64-bit prefix sums, a 128-bit product) and
// every atomic is an integer atomic: the same bits on every run.  The noise and the relocation values are evaluated in
// binary64 from the binary32 inputs and rounded once at the store (-ffp-contract=off: one IEEE operation per operator).
#include <string.h>

#include "gsr_kernels.h"

namespace gsr {

constexpr int MC_BLOCK = 256;      // rows per block of the weight scan: 256 weights of at most 2^23 fit 32 bits
constexpr int MC_RATIO_CAP = 51;   // 3DGS-MCMC's N_max: a source drawn more often is treated as drawn 50 times

// device-side state of one gsr_mcmc_sample call (the first 256 bytes of its workspace)
struct McmcState {
  gsr_mcmc_record record;  // what the host reads back
  uint32_t n_alive;
};
static_assert(sizeof(McmcState) <= 256, "McmcState must fit the workspace header");

struct McmcWork {
  McmcState* state;
  uint32_t* local;       // (P) inclusive prefix of the weights inside each block of MC_BLOCK rows
  uint32_t* block_sum;   // (nb)
  uint64_t* block_excl;  // (nb) exclusive prefix of block_sum
  void* dead_plan;       // a gsr_compact_plan workspace of dead_sel
  size_t bytes;
};
inline McmcWork carve_mcmc(void* base, int64_t P) {
  char* p = (char*)base;
  const size_t nb = ((size_t)P + MC_BLOCK - 1) / MC_BLOCK;
  McmcWork w;
  size_t off = 0;
  w.state = (McmcState*)(p + off);      off += 256;
  w.local = (uint32_t*)(p + off);       off += align_up(sizeof(uint32_t) * (size_t)P);
  w.block_sum = (uint32_t*)(p + off);   off += align_up(sizeof(uint32_t) * nb);
  w.block_excl = (uint64_t*)(p + off);  off += align_up(sizeof(uint64_t) * nb);
  w.dead_plan = (void*)(p + off);       off += align_up(compact_workspace_bytes(P));
  w.bytes = off;
  return w;
}
size_t mcmc_workspace_bytes(int64_t P) { return carve_mcmc(nullptr, P).bytes; }
const gsr_mcmc_record* mcmc_record_ptr(void* workspace, int64_t P) { return &carve_mcmc(workspace, P).state->record; }

// ---------------------------------------------------------------------------------------------------------------------
// 1. the noise of every step: xyz += Sigma (noise * g * scaler), Sigma = R diag(s^2) R^T, g = 1 / (1 + exp(k (o - (1 - x0))))
//    One thread per row; 68 bytes of traffic per row (xyz read and written, scaling, rotation, opacity, noise).  Rows are
//    12 / 16 / 4 bytes: one dwordx3 / dwordx4 / dword access each.
// ---------------------------------------------------------------------------------------------------------------------
struct alignas(4) McF3 {
  float x, y, z;
};

__global__ void __launch_bounds__(MC_BLOCK) mcmc_noise_kernel(int64_t P, float* __restrict__ xyz,
                                                             const float* __restrict__ scaling_raw,
                                                             const float* __restrict__ rotation_raw,
                                                             const float* __restrict__ opacity_raw,
                                                             const float* __restrict__ noise, const uint8_t* __restrict__ mask,
                                                             double k, double x0, double scaler) {
  const int64_t i = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= P) return;
  if (mask != nullptr && mask[i] == 0) return;  // frozen rows: nothing of them is read or written
  const McF3 x = reinterpret_cast<const McF3*>(xyz)[i];
  const McF3 sr = reinterpret_cast<const McF3*>(scaling_raw)[i];
  const McF3 nz = reinterpret_cast<const McF3*>(noise)[i];
  const float4 rot = reinterpret_cast<const float4*>(rotation_raw)[i];
  const double o = 1.0 / (1.0 + exp(-(double)opacity_raw[i]));
  const double g = 1.0 / (1.0 + exp(k * (o - (1.0 - x0))));
  const double s0 = exp((double)sr.x), s1 = exp((double)sr.y), s2 = exp((double)sr.z);
  const double r0 = rot.x, r1 = rot.y, r2 = rot.z, r3 = rot.w;
  const double n = sqrt(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3);
  const double qr = r0 / n, qx = r1 / n, qy = r2 / n, qz = r3 / n;
  double R[3][3];  // build_rotation, as densify_split_kernel writes it
  R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[0][1] = 2.0 * (qx * qy - qr * qz);
  R[0][2] = 2.0 * (qx * qz + qr * qy);
  R[1][0] = 2.0 * (qx * qy + qr * qz);
  R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[1][2] = 2.0 * (qy * qz - qr * qx);
  R[2][0] = 2.0 * (qx * qz - qr * qy);
  R[2][1] = 2.0 * (qy * qz + qr * qx);
  R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
  const double v0 = ((double)nz.x * g) * scaler, v1 = ((double)nz.y * g) * scaler, v2 = ((double)nz.z * g) * scaler;
  // Sigma v = R (s^2 * (R^T v))
  const double w0 = (s0 * s0) * ((R[0][0] * v0 + R[1][0] * v1) + R[2][0] * v2);
  const double w1 = (s1 * s1) * ((R[0][1] * v0 + R[1][1] * v1) + R[2][1] * v2);
  const double w2 = (s2 * s2) * ((R[0][2] * v0 + R[1][2] * v1) + R[2][2] * v2);
  McF3 out;
  out.x = (float)((double)x.x + ((R[0][0] * w0 + R[0][1] * w1) + R[0][2] * w2));
  out.y = (float)((double)x.y + ((R[1][0] * w0 + R[1][1] * w1) + R[1][2] * w2));
  out.z = (float)((double)x.z + ((R[2][0] * w0 + R[2][1] * w1) + R[2][2] * w2));
  reinterpret_cast<McF3*>(xyz)[i] = out;
}

hipError_t launch_mcmc_noise(hipStream_t s, int64_t P, float* xyz, const float* scaling_raw, const float* rotation_raw,
                             const float* opacity_raw, const float* noise, const uint8_t* mask, double k, double x0,
                             double scaler) {
  hipLaunchKernelGGL(mcmc_noise_kernel, dim3((unsigned)((P + MC_BLOCK - 1) / MC_BLOCK)), dim3(MC_BLOCK), 0, s, P, xyz,
                     scaling_raw, rotation_raw, opacity_raw, noise, mask, k, x0, scaler);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. classification and the draws
// ---------------------------------------------------------------------------------------------------------------------
// dead / alive, the weight k = trunc(opacity * 2^23) of an alive row, its inclusive prefix inside the block, the block's
// sum; count[] cleared.  A NaN opacity fails both comparisons: neither dead nor alive.
__global__ void __launch_bounds__(MC_BLOCK) mcmc_classify_kernel(int64_t P, const float* __restrict__ opacity,
                                                                const uint8_t* __restrict__ mask, float min_opacity,
                                                                uint8_t* __restrict__ dead_sel, int32_t* __restrict__ count,
                                                                uint32_t* __restrict__ local, uint32_t* __restrict__ block_sum,
                                                                McmcState* __restrict__ st) {
  __shared__ uint32_t smem[MC_BLOCK / 64 + 1];
  __shared__ uint32_t alive_sh;
  if (threadIdx.x == 0) alive_sh = 0;
  const int64_t i = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  uint32_t k = 0;
  bool alive = false;
  if (i < P) {
    const float o = opacity[i];
    const bool m = mask == nullptr || mask[i] != 0;
    const bool dead = m && o <= min_opacity;
    alive = m && o > min_opacity;
    dead_sel[i] = dead ? 1 : 0;
    count[i] = 0;
    if (alive) {
      const float w = o * 8388608.0f;  // exact: a power of two
      k = w >= 8388608.0f ? 8388608u : (uint32_t)w;  // (an opacity above 1, infinity included, weighs as 1)
    }
  }
  uint32_t total;
  const uint32_t ex = block_excl_scan_u32<MC_BLOCK>(k, &total, smem);
  if (i < P) local[i] = ex + k;
  const uint32_t wave_alive = (uint32_t)__popcll(__ballot(alive));
  if ((threadIdx.x & 63) == 0 && wave_alive != 0) atomicAdd(&alive_sh, wave_alive);
  __syncthreads();
  if (threadIdx.x == 0) {
    block_sum[blockIdx.x] = total;
    if (alive_sh != 0) atomicAdd(&st->n_alive, alive_sh);
  }
}

// One block: the exclusive 64-bit prefix of the block sums, each thread a contiguous run of them; then the record.
__global__ void __launch_bounds__(MC_BLOCK) mcmc_scan_kernel(int64_t nb, const uint32_t* __restrict__ block_sum,
                                                            uint64_t* __restrict__ block_excl, McmcState* __restrict__ st,
                                                            const uint64_t* __restrict__ n_dead, int64_t n, int draws_from_dead) {
  __shared__ uint64_t part[MC_BLOCK];
  const int64_t run = (nb + MC_BLOCK - 1) / MC_BLOCK;
  const int64_t lo = min(nb, (int64_t)threadIdx.x * run), hi = min(nb, lo + run);
  uint64_t sum = 0;
  for (int64_t b = lo; b < hi; ++b) sum += block_sum[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t carry = 0;
    for (int t = 0; t < MC_BLOCK; ++t) {
      const uint64_t v = part[t];
      part[t] = carry;
      carry += v;
    }
    const int64_t dead = (int64_t)*n_dead;
    st->record.n_dead = dead;
    st->record.n_alive = (int64_t)st->n_alive;
    st->record.n_draws = draws_from_dead ? (dead < n ? dead : n) : n;
    st->record.total = carry;
  }
  __syncthreads();
  uint64_t carry = part[threadIdx.x];
  for (int64_t b = lo; b < hi; ++b) {
    block_excl[b] = carry;
    carry += block_sum[b];
  }
}

// draw r: m = u 2^24, t = (m total) >> 24 from the 128-bit product, src = the smallest j with S_j > t.  t < total because
// m < 2^24, so the row exists whenever total > 0; it is found by two binary searches (blocks, then rows of the block).
__global__ void __launch_bounds__(MC_BLOCK) mcmc_draw_kernel(int64_t P, int64_t n, const float* __restrict__ u,
                                                            const McmcState* __restrict__ st,
                                                            const uint32_t* __restrict__ local,
                                                            const uint64_t* __restrict__ block_excl, int32_t* __restrict__ src,
                                                            int32_t* __restrict__ count) {
  const int64_t r = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (r >= n) return;
  const uint64_t total = st->record.total;
  if (r >= st->record.n_draws || total == 0) {
    src[r] = -1;
    return;
  }
  float uu = u[r];
  uu = uu >= 0.0f ? uu : 0.0f;  // (NaN and negative numbers draw as 0, 1 and above as the largest u)
  const float mf = uu * 16777216.0f;
  const uint64_t m = mf >= 16777215.0f ? 16777215ull : (uint64_t)mf;
  const uint64_t t = (__umul64hi(m, total) << 40) | ((m * total) >> 24);
  const int64_t nb = (P + MC_BLOCK - 1) / MC_BLOCK;
  int64_t lo = 0, hi = nb - 1;  // the largest block b with block_excl[b] <= t (it is not empty: see DESIGN.md)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (block_excl[mid] <= t) lo = mid; else hi = mid - 1;
  }
  const uint32_t rem = (uint32_t)(t - block_excl[lo]);
  const int64_t row0 = lo * MC_BLOCK;
  int a = 0, b = (int)min((int64_t)MC_BLOCK, P - row0) - 1;  // the smallest row of the block with local > rem
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (local[row0 + mid] > rem) b = mid; else a = mid + 1;
  }
  const int64_t j = row0 + a;
  src[r] = (int32_t)j;
  atomicAdd(&count[j], 1);
}

__global__ void __launch_bounds__(MC_BLOCK) mcmc_ratio_kernel(int64_t n, const int32_t* __restrict__ src,
                                                             const int32_t* __restrict__ count, int32_t* __restrict__ ratio) {
  const int64_t r = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (r >= n) return;
  const int32_t s = src[r];
  ratio[r] = s < 0 ? 0 : min(count[s] + 1, MC_RATIO_CAP);
}

hipError_t launch_mcmc_sample(hipStream_t s, int64_t P, int64_t n, const float* opacity, const uint8_t* mask,
                              float min_opacity, const float* u, int draws_from_dead, void* workspace, uint8_t* dead_sel,
                              int32_t* dead_idx, int32_t* src, int32_t* count, int32_t* ratio) {
  const McmcWork w = carve_mcmc(workspace, P);
  const int64_t nb = (P + MC_BLOCK - 1) / MC_BLOCK;
  hipError_t e = hipMemsetAsync(w.state, 0, 256, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mcmc_classify_kernel, dim3((unsigned)nb), dim3(MC_BLOCK), 0, s, P, opacity, mask, min_opacity, dead_sel,
                     count, w.local, w.block_sum, w.state);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_compact_plan(s, P, dead_sel, w.dead_plan)) != hipSuccess) return e;
  const gsr_compact_tensor iota = {nullptr, dead_idx, 4};  // the dead rows' numbers, ascending
  if ((e = launch_compact_apply(s, P, dead_sel, w.dead_plan, 1, &iota)) != hipSuccess) return e;
  hipLaunchKernelGGL(mcmc_scan_kernel, dim3(1), dim3(MC_BLOCK), 0, s, nb, w.block_sum, w.block_excl, w.state,
                     compact_total_ptr(w.dead_plan, P), n, draws_from_dead);
  if (n > 0) {
    const unsigned grid = (unsigned)((n + MC_BLOCK - 1) / MC_BLOCK);
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3(grid), dim3(MC_BLOCK), 0, s, P, n, u, w.state, w.local, w.block_excl, src, count);
    hipLaunchKernelGGL(mcmc_ratio_kernel, dim3(grid), dim3(MC_BLOCK), 0, s, n, src, count, ratio);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. the relocation values of draw r (source s, n = ratio[r]), binary64 throughout, rounded at the two stores:
//      o = min(opacity_s, 1 - 2^-24); o' = 1 - (1 - o)^(1/n)
//      denom = sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1), in this order, o'^(k+1) by repeated product
//      scale' = exp(scaling_raw_s) o / denom;  o' clamped to [min_opacity, 1 - 2^-23]
//    Only OLD values are read and only draw-indexed temporaries are written: a source drawn several times gives every one
//    of its draws the same numbers.
// ---------------------------------------------------------------------------------------------------------------------
struct McmcBinom {
  double c[MC_RATIO_CAP][MC_RATIO_CAP];
};
constexpr McmcBinom make_binom() {  // Pascal's triangle; every entry is below 2^53, so the sums are exact
  McmcBinom b = {};
  for (int i = 0; i < MC_RATIO_CAP; ++i) {
    b.c[i][0] = 1.0;
    for (int k = 1; k <= i; ++k) b.c[i][k] = b.c[i - 1][k - 1] + (k <= i - 1 ? b.c[i - 1][k] : 0.0);
  }
  return b;
}
__constant__ McmcBinom mcmc_binom = make_binom();

__global__ void __launch_bounds__(MC_BLOCK) mcmc_values_kernel(int64_t P, int64_t n, const int32_t* __restrict__ src,
                                                              const int32_t* __restrict__ ratio,
                                                              const float* __restrict__ opacity,
                                                              const float* __restrict__ scaling_raw, float min_opacity,
                                                              float* __restrict__ new_opacity_raw,
                                                              float* __restrict__ new_scaling_raw) {
  __shared__ double root[MC_RATIO_CAP];
  if (threadIdx.x < MC_RATIO_CAP) root[threadIdx.x] = sqrt((double)(threadIdx.x + 1));
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (r >= n) return;
  const int64_t s = src[r];
  if (s < 0 || s >= P) {  // no draw (total == 0, or beyond n_draws): zeros, which the scatter never reads
    new_opacity_raw[r] = 0.0f;
    new_scaling_raw[3 * r] = new_scaling_raw[3 * r + 1] = new_scaling_raw[3 * r + 2] = 0.0f;
    return;
  }
  const int N = min(max(ratio[r], 1), MC_RATIO_CAP);
  const double o = fmin((double)opacity[s], 1.0 - 0x1p-24);
  double op = 1.0 - pow(1.0 - o, 1.0 / (double)N);
  double denom = 0.0;
  for (int i = 1; i <= N; ++i) {
    double p = op;
    for (int k = 0; k < i; ++k) {
      const double term = (mcmc_binom.c[i - 1][k] * p) / root[k];
      denom = (k & 1) ? denom - term : denom + term;
      p = p * op;
    }
  }
  const double f = o / denom;
  op = fmin(fmax(op, (double)min_opacity), 1.0 - 0x1p-23);
  new_opacity_raw[r] = (float)log(op / (1.0 - op));
  for (int c = 0; c < 3; ++c) new_scaling_raw[3 * r + c] = (float)log(exp((double)scaling_raw[3 * s + c]) * f);
}

hipError_t launch_mcmc_values(hipStream_t s, int64_t P, int64_t n, const int32_t* src, const int32_t* ratio,
                              const float* opacity, const float* scaling_raw, float min_opacity, float* new_opacity_raw,
                              float* new_scaling_raw) {
  hipLaunchKernelGGL(mcmc_values_kernel, dim3((unsigned)((n + MC_BLOCK - 1) / MC_BLOCK)), dim3(MC_BLOCK), 0, s, P, n, src, ratio,
                     opacity, scaling_raw, min_opacity, new_opacity_raw, new_scaling_raw);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// 4. the scatter of relocation and growth, one launch per role for all tensors of that role.  Draw r has the source row s = src[r] of `base`
//    and the destination row d = dst_idx[r] (relocation: the r-th dead row of the same tensor) or r (growth: a buffer of
//    the appended rows).  COPY: dst[d] = base[s].  VALUE: dst[d] = base[s] = values[r].  ZERO: base[s] = 0.
//    Sources are alive and destinations dead or outside `base`, so no row is both read and written; the draws of one
//    source carry identical values, so their stores to base[s] agree.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MC_MAX_TENSORS = 32;
struct McmcTensorDev {
  uint32_t* base;
  uint32_t* dst;
  const uint32_t* values;
  uint32_t words;
  int32_t role;
};
struct McmcScatterArgs {
  McmcTensorDev t[MC_MAX_TENSORS];
  int64_t P, n, dst_rows;
  const int32_t* src;
  const int32_t* dst_idx;
};

// grid = (blocks over the draws' words, tensors of this role).  One instantiation per role: straight-line code with the
// role's one or two stores, every address formed from the tensor's own pointers.
template <int ROLE>
__global__ void __launch_bounds__(MC_BLOCK) mcmc_scatter_kernel(const McmcScatterArgs a) {
  const McmcTensorDev t = a.t[blockIdx.y];
  const uint64_t W = t.words, total = (uint64_t)a.n * W, stride = (uint64_t)gridDim.x * MC_BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x; e < total; e += stride) {
    const uint64_t r = e / W, c = e - r * W;
    const int64_t s = a.src[r];
    if (s < 0 || s >= a.P) continue;
    uint32_t* const from = t.base + ((uint64_t)s * W + c);
    if (ROLE == GSR_MCMC_ZERO) {
      *from = 0u;
      continue;
    }
    const int64_t d = a.dst_idx != nullptr ? (int64_t)a.dst_idx[r] : (int64_t)r;
    const bool d_ok = d >= 0 && d < a.dst_rows;
    uint32_t* const to = t.dst + ((uint64_t)(d_ok ? d : 0) * W + c);
    if (ROLE == GSR_MCMC_COPY) {
      if (d_ok) *to = *from;
    } else {
      const uint32_t v = t.values[e];
      if (d_ok) *to = v;
      *from = v;
    }
  }
}

hipError_t launch_mcmc_scatter(hipStream_t s, int64_t P, int64_t n, const int32_t* src, const int32_t* dst_idx,
                               int64_t dst_rows, int nt, const gsr_mcmc_tensor* tensors) {
  if (nt <= 0 || n <= 0 || P <= 0) return hipSuccess;
  if (nt > MC_MAX_TENSORS) return hipErrorInvalidValue;
  for (int role = GSR_MCMC_COPY; role <= GSR_MCMC_ZERO; ++role) {  // one launch per role in use
    McmcScatterArgs a;
    memset(&a, 0, sizeof(a));
    a.P = P;
    a.n = n;
    a.dst_rows = dst_rows;
    a.src = src;
    a.dst_idx = dst_idx;
    uint64_t most = 0;
    int k = 0;
    for (int i = 0; i < nt; ++i) {
      if (tensors[i].role != role) continue;
      a.t[k].base = (uint32_t*)tensors[i].base;
      a.t[k].dst = (uint32_t*)tensors[i].dst;
      a.t[k].values = (const uint32_t*)tensors[i].values;
      a.t[k].words = (uint32_t)(tensors[i].row_bytes >> 2);
      a.t[k].role = role;
      const uint64_t words = (uint64_t)n * a.t[k].words;
      if (words > most) most = words;
      ++k;
    }
    if (k == 0) continue;
    const uint64_t want = (most + MC_BLOCK - 1) / MC_BLOCK;
    const dim3 grid((unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want)), (unsigned)k);
    if (role == GSR_MCMC_COPY) hipLaunchKernelGGL(mcmc_scatter_kernel<GSR_MCMC_COPY>, grid, dim3(MC_BLOCK), 0, s, a);
    else if (role == GSR_MCMC_VALUE) hipLaunchKernelGGL(mcmc_scatter_kernel<GSR_MCMC_VALUE>, grid, dim3(MC_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(mcmc_scatter_kernel<GSR_MCMC_ZERO>, grid, dim3(MC_BLOCK), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace gsr
