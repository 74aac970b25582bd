// gsr_densify.hip -- the densification POLICY of the editor's loop: the per-step statistics, the
// clone / split decision with its quantile threshold, the positions of the split children and the prune mask.
//
// The reference runs all of it with torch ops over P rows: on_before_optimizer_step (threestudio/systems/
// GassuianEditor.py:251-281) + add_densification_stats (gaussiansplatting/scene/gaussian_model.py:811-815) every step,
// densify_and_prune (:768-809) with densify_and_clone (:730-766) and densify_and_split (:673-728) every
// densification_interval steps: boolean-mask indexing (nonzero + host sync each), torch.quantile (a full sort of P floats),
// repeat, bmm.  Here: one launch for the statistics, no readback; the decision as a handful of launches with ONE readback.
// Every float operation below is a single binary32 operation in the order the reference's lines evaluate it
// (-ffp-contract=off; fmaf only where torch's lerp fuses), and every atomic is an integer atomic: the same bits each run.
#include <string.h>

#include "gsr_kernels.h"

namespace gsr {

constexpr int DNS_BLOCK = 256;
constexpr int DNS_MAX_BLOCKS = 1024;  // grid-stride kernels: at most this many blocks

// device-side state of one gsr_densify_select call (the first 256 bytes of its workspace)
struct DensifyState {
  gsr_densify_result result;  // what the host reads back
  uint32_t nnz;               // #{g != 0}
  uint32_t prefix[2];         // radix select of the lo-th / hi-th smallest key: the digits found so far ...
  uint32_t remaining[2];      // ... and the rank inside the keys that share them
  float w;                    // the quantile's interpolation weight
  float threshold;
};
static_assert(sizeof(DensifyState) <= 256, "DensifyState must fit the workspace header");

struct DensifyWork {
  DensifyState* state;
  uint32_t* hist;  // (4 passes, 2 selects, 256 bins)
  float* g;        // (P) the materialised gradient statistic
  void* clone_plan;  // a gsr_compact_plan workspace each
  void* split_plan;
  size_t bytes;
};
inline DensifyWork carve_densify(void* base, int64_t P) {
  char* p = (char*)base;
  DensifyWork w;
  size_t off = 0;
  w.state = (DensifyState*)(p + off);  off += 256;
  w.hist = (uint32_t*)(p + off);       off += align_up(sizeof(uint32_t) * 4 * 2 * 256);
  w.g = (float*)(p + off);             off += align_up(sizeof(float) * (size_t)P);
  w.clone_plan = (void*)(p + off);     off += align_up(compact_workspace_bytes(P));
  w.split_plan = (void*)(p + off);     off += align_up(compact_workspace_bytes(P));
  w.bytes = off;
  return w;
}
size_t densify_workspace_bytes(int64_t P) { return carve_densify(nullptr, P).bytes; }
void densify_plans(void* workspace, int64_t P, void** clone_plan, void** split_plan) {
  const DensifyWork w = carve_densify(workspace, P);
  *clone_plan = w.clone_plan;
  *split_plan = w.split_plan;
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. the per-step statistics: GassuianEditor.py:254-261 (the views' gradients summed in view order, radii = max over the
//    views), :271-273 (max_radii2D[vis] = max(max_radii2D[vis], radii[vis])), gaussian_model.py:811-815
// ---------------------------------------------------------------------------------------------------------------------
struct StatsArgs {
  const float* grad[8];
  const int32_t* radii[8];
  int V;
  int64_t P;
  float* accum;
  float* denom;
  float* max_radii;
};

__global__ void __launch_bounds__(DNS_BLOCK) densify_stats_kernel(const StatsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * DNS_BLOCK + threadIdx.x;
  if (i >= a.P) return;
  int32_t r = a.radii[0][i];
  for (int v = 1; v < a.V; ++v) r = max(r, a.radii[v][i]);
  if (r <= 0) return;  // not in update_filter: nothing of this row is read or written
  float gx = 0.0f, gy = 0.0f;
  for (int v = 0; v < a.V; ++v) {
    gx = gx + a.grad[v][3 * i + 0];
    gy = gy + a.grad[v][3 * i + 1];
  }
  a.accum[i] = a.accum[i] + sqrtf(gx * gx + gy * gy);
  a.denom[i] = a.denom[i] + 1.0f;
  a.max_radii[i] = fmaxf(a.max_radii[i], (float)r);
}

hipError_t launch_densify_stats(hipStream_t s, int64_t P, int V, const float* const* grads, const int32_t* const* radii,
                                float* accum, float* denom, float* max_radii) {
  StatsArgs a;
  memset(&a, 0, sizeof(a));
  for (int v = 0; v < V; ++v) {
    a.grad[v] = grads[v];
    a.radii[v] = radii[v];
  }
  a.V = V;
  a.P = P;
  a.accum = accum;
  a.denom = denom;
  a.max_radii = max_radii;
  hipLaunchKernelGGL(densify_stats_kernel, dim3((unsigned)((P + DNS_BLOCK - 1) / DNS_BLOCK)), dim3(DNS_BLOCK), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. the decision of densify_and_prune (:771-777), densify_and_clone (:732-739) and densify_and_split (:676-683)
// ---------------------------------------------------------------------------------------------------------------------
// order-preserving integer image of a float (no NaN arrives here): a < b  <=>  key(a) < key(b), -0 below +0
__device__ __forceinline__ uint32_t float_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// g = accum / denom, NaN -> 0, unmasked -> 0 (:771-773), materialised; nnz; the histogram of the keys' top byte
__global__ void __launch_bounds__(DNS_BLOCK) densify_grad_kernel(int64_t P, const float* __restrict__ accum,
                                                                const float* __restrict__ denom,
                                                                const uint8_t* __restrict__ mask, float* __restrict__ g_out,
                                                                DensifyState* __restrict__ st, uint32_t* __restrict__ hist,
                                                                int want_hist) {
  __shared__ uint32_t lh[256];
  __shared__ uint32_t lnnz;
  lh[threadIdx.x] = 0;
  if (threadIdx.x == 0) lnnz = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * DNS_BLOCK;
  uint32_t my_nnz = 0;
  for (int64_t i = (int64_t)blockIdx.x * DNS_BLOCK + threadIdx.x; i < P; i += stride) {
    float g = accum[i] / denom[i];
    if (g != g) g = 0.0f;
    if (mask[i] == 0) g = 0.0f;
    g_out[i] = g;
    my_nnz += (g != 0.0f) ? 1u : 0u;
    if (want_hist) atomicAdd(&lh[float_key(g) >> 24], 1u);
  }
  if (my_nnz != 0) atomicAdd(&lnnz, my_nnz);
  __syncthreads();
  if (threadIdx.x == 0 && lnnz != 0) atomicAdd(&st->nnz, lnnz);
  if (want_hist && lh[threadIdx.x] != 0) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

// pass = 1..3: per select, the histogram of the next byte over the keys that share the digits found so far
__global__ void __launch_bounds__(DNS_BLOCK) densify_hist_kernel(int64_t P, const float* __restrict__ g, int pass,
                                                                const DensifyState* __restrict__ st,
                                                                uint32_t* __restrict__ hist /* this pass: (2, 256) */) {
  __shared__ uint32_t lh[2][256];
  lh[0][threadIdx.x] = 0;
  lh[1][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t p0 = st->prefix[0], p1 = st->prefix[1];
  const int hi_shift = 32 - 8 * pass, lo_shift = 24 - 8 * pass;
  const int64_t stride = (int64_t)gridDim.x * DNS_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * DNS_BLOCK + threadIdx.x; i < P; i += stride) {
    const uint32_t key = float_key(g[i]);
    const uint32_t top = key >> hi_shift, digit = (key >> lo_shift) & 255u;
    if (top == p0) atomicAdd(&lh[0][digit], 1u);
    if (top == p1) atomicAdd(&lh[1][digit], 1u);
  }
  __syncthreads();
  if (lh[0][threadIdx.x] != 0) atomicAdd(&hist[threadIdx.x], lh[0][threadIdx.x]);
  if (lh[1][threadIdx.x] != 0) atomicAdd(&hist[256 + threadIdx.x], lh[1][threadIdx.x]);
}

// One block.  pass 0 first turns nnz into the two ranks (:775-776 and torch.quantile's rank arithmetic); every pass then
// finds, per select, the bin that holds its rank; pass 3 ends with the threshold (torch's two-sided lerp).
__global__ void __launch_bounds__(DNS_BLOCK) densify_pick_kernel(int64_t P, int pass, double max_densify_percent,
                                                                DensifyState* st,
                                                                const uint32_t* __restrict__ hist /* this pass: (2, 256) */) {
  __shared__ uint32_t smem[DNS_BLOCK / 64 + 1];
  __shared__ uint32_t rank_sh[2];
  if (pass == 0 && threadIdx.x == 0) {
    const double vp = (double)st->nnz * max_densify_percent / (double)P;
    const float q = (float)(1.0 - vp);
    const float rank = q * (float)(P - 1);
    float lo = floorf(rank);
    if (!(lo >= 0.0f)) lo = 0.0f;
    if (lo > (float)(P - 1)) lo = (float)(P - 1);
    st->w = rank - lo;
    const uint32_t l = (uint32_t)lo;
    rank_sh[0] = l;
    rank_sh[1] = (int64_t)l + 1 < P ? l + 1u : (uint32_t)(P - 1);
  } else if (pass != 0 && threadIdx.x < 2) {
    rank_sh[threadIdx.x] = st->remaining[threadIdx.x];
  }
  __syncthreads();
  for (int s = 0; s < 2; ++s) {
    const uint32_t* h = hist + (pass == 0 ? 0 : 256 * s);  // the first pass has no digits yet: one histogram serves both
    const uint32_t c = h[threadIdx.x];
    uint32_t total;
    const uint32_t ex = block_excl_scan_u32<DNS_BLOCK>(c, &total, smem);
    const uint32_t k = rank_sh[s];
    if (c != 0 && ex <= k && k < ex + c) {  // exactly one bin
      st->prefix[s] = pass == 0 ? threadIdx.x : ((st->prefix[s] << 8) | threadIdx.x);
      st->remaining[s] = k - ex;
    }
    __syncthreads();
  }
  if (pass == 3 && threadIdx.x == 0) {
    const float a = key_float(st->prefix[0]), b = key_float(st->prefix[1]);
    const float w = st->w;
    const float t = w < 0.5f ? fmaf(w, b - a, a) : fmaf(w - 1.0f, b - a, b);
    st->threshold = t;
  }
}

__global__ void __launch_bounds__(DNS_BLOCK) densify_decide_kernel(int64_t P, const float* __restrict__ g,
                                                                  const float* __restrict__ scaling, int use_threshold,
                                                                  const DensifyState* __restrict__ st, float max_grad,
                                                                  float t_dense, uint8_t* __restrict__ clone_sel,
                                                                  uint8_t* __restrict__ split_sel) {
  const int64_t i = (int64_t)blockIdx.x * DNS_BLOCK + threadIdx.x;
  if (i >= P) return;
  float v = g[i];
  if (use_threshold && v < st->threshold) v = 0.0f;  // :777
  float m = scaling[3 * i];
  m = fmaxf(m, scaling[3 * i + 1]);
  m = fmaxf(m, scaling[3 * i + 2]);
  const bool hot = v >= max_grad;
  clone_sel[i] = (hot && m <= t_dense) ? 1 : 0;
  split_sel[i] = (hot && m > t_dense) ? 1 : 0;
}

__global__ void densify_result_kernel(DensifyState* __restrict__ st, int use_threshold, const uint64_t* __restrict__ n_clone,
                                      const uint64_t* __restrict__ n_split) {
  st->result.nonzero = (int64_t)st->nnz;
  st->result.n_clone = (int64_t)*n_clone;
  st->result.n_split = (int64_t)*n_split;
  st->result.threshold = use_threshold ? st->threshold : 0.0f;
}

hipError_t launch_densify_select(hipStream_t s, int64_t P, const float* accum, const float* denom, const uint8_t* mask,
                                 const float* scaling, float max_grad, double max_densify_percent, float t_dense,
                                 void* workspace, uint8_t* clone_sel, uint8_t* split_sel) {
  const DensifyWork w = carve_densify(workspace, P);
  const int use_threshold = max_densify_percent < 1.0 ? 1 : 0;
  const int64_t nb = (P + DNS_BLOCK - 1) / DNS_BLOCK;
  const unsigned grid = (unsigned)(nb < DNS_MAX_BLOCKS ? nb : DNS_MAX_BLOCKS);
  hipError_t e = hipMemsetAsync(w.state, 0, 256 + sizeof(uint32_t) * 4 * 2 * 256, s);  // state and histograms are adjacent
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(densify_grad_kernel, dim3(grid), dim3(DNS_BLOCK), 0, s, P, accum, denom, mask, w.g, w.state, w.hist,
                     use_threshold);
  if (use_threshold) {
    for (int pass = 0; pass < 4; ++pass) {
      uint32_t* h = w.hist + 512 * pass;
      if (pass > 0) hipLaunchKernelGGL(densify_hist_kernel, dim3(grid), dim3(DNS_BLOCK), 0, s, P, w.g, pass, w.state, h);
      hipLaunchKernelGGL(densify_pick_kernel, dim3(1), dim3(DNS_BLOCK), 0, s, P, pass, max_densify_percent, w.state, h);
    }
  }
  hipLaunchKernelGGL(densify_decide_kernel, dim3((unsigned)nb), dim3(DNS_BLOCK), 0, s, P, w.g, scaling, use_threshold, w.state,
                     max_grad, t_dense, clone_sel, split_sel);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_compact_plan(s, P, clone_sel, w.clone_plan)) != hipSuccess) return e;
  if ((e = launch_compact_plan(s, P, split_sel, w.split_plan)) != hipSuccess) return e;
  hipLaunchKernelGGL(densify_result_kernel, dim3(1), dim3(1), 0, s, w.state, use_threshold,
                     compact_total_ptr(w.clone_plan, P), compact_total_ptr(w.split_plan, P));
  return hipGetLastError();
}
const gsr_densify_result* densify_result_ptr(void* workspace, int64_t P) { return &carve_densify(workspace, P).state->result; }

// ---------------------------------------------------------------------------------------------------------------------
// 3. positions of the split children (:685-691): build_rotation (utils/general_utils.py:78-99) of the raw quaternion,
//    times the sample, plus the parent's position.  One thread per ORIGINAL row; a selected row finds its rank among the
//    selected ones from the plan of split_sel (block offsets of 1024-row blocks) and a scan inside its block.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SPLIT_ROWS = VIEW_MSG_ROWS;  // == the compaction's block

__global__ void __launch_bounds__(SPLIT_ROWS) densify_split_kernel(int64_t P, const float* __restrict__ xyz,
                                                                  const float* __restrict__ scaling,
                                                                  const float* __restrict__ rotation,
                                                                  const uint8_t* __restrict__ sel,
                                                                  const uint32_t* __restrict__ block_off, int64_t n_split, int N,
                                                                  const float* __restrict__ noise, float* __restrict__ out) {
  __shared__ uint32_t smem[SPLIT_ROWS / 64 + 1];
  const int64_t i = (int64_t)blockIdx.x * SPLIT_ROWS + threadIdx.x;
  const uint32_t k = (i < P && sel[i] != 0) ? 1u : 0u;
  uint32_t total;
  const uint32_t ex = block_excl_scan_u32<SPLIT_ROWS>(k, &total, smem);
  if (!k) return;
  const int64_t r = (int64_t)block_off[blockIdx.x] + ex;
  if (r >= n_split) return;  // (a plan that does not belong to sel: never write outside the outputs)
  const float r0 = rotation[4 * i], r1 = rotation[4 * i + 1], r2 = rotation[4 * i + 2], r3 = rotation[4 * i + 3];
  const float n = sqrtf(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3);
  const float qr = r0 / n, qx = r1 / n, qy = r2 / n, qz = r3 / n;
  float R[3][3];
  R[0][0] = 1.0f - 2.0f * (qy * qy + qz * qz);
  R[0][1] = 2.0f * (qx * qy - qr * qz);
  R[0][2] = 2.0f * (qx * qz + qr * qy);
  R[1][0] = 2.0f * (qx * qy + qr * qz);
  R[1][1] = 1.0f - 2.0f * (qx * qx + qz * qz);
  R[1][2] = 2.0f * (qy * qz - qr * qx);
  R[2][0] = 2.0f * (qx * qz - qr * qy);
  R[2][1] = 2.0f * (qy * qz + qr * qx);
  R[2][2] = 1.0f - 2.0f * (qx * qx + qy * qy);
  const float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
  const float x0 = xyz[3 * i], x1 = xyz[3 * i + 1], x2 = xyz[3 * i + 2];
  for (int c = 0; c < N; ++c) {
    const int64_t row = (int64_t)c * n_split + r;  // .repeat(N, 1) order
    const float a0 = noise[3 * row] * s0, a1 = noise[3 * row + 1] * s1, a2 = noise[3 * row + 2] * s2;
    out[3 * row + 0] = ((R[0][0] * a0 + R[0][1] * a1) + R[0][2] * a2) + x0;
    out[3 * row + 1] = ((R[1][0] * a0 + R[1][1] * a1) + R[1][2] * a2) + x1;
    out[3 * row + 2] = ((R[2][0] * a0 + R[2][1] * a1) + R[2][2] * a2) + x2;
  }
}

hipError_t launch_densify_split_xyz(hipStream_t s, int64_t P, const float* xyz, const float* scaling, const float* rotation,
                                    const uint8_t* split_sel, void* split_plan, int64_t n_split, int N, const float* noise,
                                    float* new_xyz) {
  const int64_t nb = (P + SPLIT_ROWS - 1) / SPLIT_ROWS;
  hipLaunchKernelGGL(densify_split_kernel, dim3((unsigned)nb), dim3(SPLIT_ROWS), 0, s, P, xyz, scaling, rotation, split_sel,
                     compact_block_off_ptr(split_plan, P), n_split, N, noise, new_xyz);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// 4. the prune mask (:787-794) together with the split parents' removal (:720-727), as a KEEP mask
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DNS_BLOCK) densify_keep_kernel(int64_t P, const float* __restrict__ opacity,
                                                                const float* __restrict__ scaling,
                                                                const float* __restrict__ max_radii,
                                                                const uint8_t* __restrict__ mask, const uint8_t* __restrict__ drop,
                                                                float min_opacity, float max_screen, float big_ws,
                                                                uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * DNS_BLOCK + threadIdx.x;
  if (i >= P) return;
  float m = scaling[3 * i];
  m = fmaxf(m, scaling[3 * i + 1]);
  m = fmaxf(m, scaling[3 * i + 2]);
  bool prune = opacity[i] < min_opacity;
  if (max_radii != nullptr) prune = prune || max_radii[i] > max_screen;
  prune = prune || m > big_ws;
  prune = prune && mask[i] != 0;
  const bool dropped = drop != nullptr && drop[i] != 0;
  keep[i] = (!dropped && !prune) ? 1 : 0;
}

hipError_t launch_densify_keep(hipStream_t s, int64_t P, const float* opacity, const float* scaling, const float* max_radii,
                               const uint8_t* mask, const uint8_t* drop, float min_opacity, float max_screen, float big_ws,
                               uint8_t* keep) {
  hipLaunchKernelGGL(densify_keep_kernel, dim3((unsigned)((P + DNS_BLOCK - 1) / DNS_BLOCK)), dim3(DNS_BLOCK), 0, s, P, opacity,
                     scaling, max_radii, mask, drop, min_opacity, max_screen, big_ws, keep);
  return hipGetLastError();
}

}  // namespace gsr
