// gsr_pose.hip -- the camera gradient (opt-in; include/gsr.h: gsr_pose_backward): dL/dviewmatrix, dL/dprojmatrix and
// dL/dcampos of a view, from the accumulator rows K7 left, BETWEEN the backward's two halves (K8+K9 cleans the rows).
//
// The rasterizer is a function of three camera tensors; per visible Gaussian, in the names of preprocess_backward_kernel
// (gsr_preprocess.hip), with (mu, 1) the homogeneous position and V[c][r] = viewmatrix[4 c + r]:
//   t = (mu, 1) V            dV[c][r]  += (dL_dtx, dL_dty, dL_dtz (+ dL_ddepth))_r (mu, 1)_c             r = 0..2
//   T = W J, W = V[:3,:3]^T  dV[r][k]  += sum_c dL_dT[c][r] J[c][k]                                     r, k = 0..2
//   p_hom = (mu, 1) PV       dPV[c][r] += (g2x m_w, g2y m_w, -, -(mul1 g2x + mul2 g2y))_r (mu, 1)_c
//   dir = mu - campos        dC        -= dm (the dnormvdv term K9 adds to dL_dmeans3D)
// Column 3 of the view matrix and column 2 of the projection matrix enter nothing the rasterizer computes: exact zeros.
// The conventions are those of K8+K9 (the reference's analytic backward): off-cone tx / ty are constants (x_grad_mul,
// y_grad_mul), the alpha clamp is straight-through, under AA the factor h is differentiated through the covariance.
//
// 27 sums over the Gaussians (12 + 12 + 3).  No float atomics: a thread adds its Gaussians in ascending index order, a wave
// reduces with DPP moves, the four waves of a block meet in LDS, every block stores one row of partial sums, and one
// workgroup adds the rows in ascending block order in double.  Given the same accumulator table the result is the same bits.
#include "gsr_kernels.h"

namespace gsr {

template <bool DEPTH, bool AA>
__global__ void __launch_bounds__(GAUSS_BLOCK) pose_backward_kernel(const PoseArgs a) {
  __shared__ float sh_part[GAUSS_BLOCK / 64][POSE_SUMS_PAD];
  float s[POSE_SUMS];
#pragma unroll
  for (int k = 0; k < POSE_SUMS; ++k) s[k] = 0.f;
  bool wave_any = false;  // (wave-uniform: some lane of this wave contributed)
  Cam cam;
  load_cam(cam, a.viewmatrix, a.projmatrix, a.sh ? a.campos : nullptr);
  const float* view = cam.view;
  const float* proj = cam.proj;
  typedef float acc_f4 __attribute__((ext_vector_type(4)));
  const int64_t stride = (int64_t)gridDim.x * GAUSS_BLOCK;
  for (int64_t base = (int64_t)blockIdx.x * GAUSS_BLOCK; base < a.P; base += stride) {
    const int64_t raw = base + threadIdx.x;
    const bool live = raw < a.P;
    const size_t idx = (size_t)(live ? raw : (int64_t)a.P - 1);
    // the row first: one Gaussian in ten of a view has one that is not zero, and only those cost anything more
    const acc_f4* const acc_row = reinterpret_cast<const acc_f4*>(a.acc + idx * ACC_ROW);
    const acc_f4 acc_m2d = acc_row[ACC_MEAN2D / 4], acc_con = acc_row[ACC_CONIC / 4], acc_col = acc_row[ACC_COLOR / 4];
    const int32_t radius = a.radii[idx];
    const bool nonzero = !(acc_m2d.x == 0.f) || !(acc_m2d.y == 0.f) || !(acc_m2d.w == 0.f) || !(acc_con.x == 0.f) ||
                         !(acc_con.y == 0.f) || !(acc_con.w == 0.f) || !(acc_col.x == 0.f) || !(acc_col.y == 0.f) ||
                         !(acc_col.z == 0.f) || (DEPTH && !(acc_col.w == 0.f));
    const bool on = live && radius > 0 && nonzero;
    if (__ballot(on) == 0ull) continue;  // no lane of this wave has anything to add
    wave_any = true;
    if (!on) continue;
    const V3 mean = {a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]};
    float c3[6];
    if (a.cov3D_precomp != nullptr) {
#pragma unroll
      for (int i = 0; i < 6; ++i) c3[i] = a.cov3D_precomp[6 * idx + i];
    } else {
      const float4 quat = reinterpret_cast<const float4*>(a.rotations)[idx];
      cov3d_from_values(a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2], a.scale_modifier, quat, c3);
    }
    const float aa_ow = AA ? a.rec0[idx].w : 0.f;
    const float g2x = acc_m2d.x, g2y = acc_m2d.y;
    const V3 dL_dcon = {acc_con.x, acc_con.y, acc_con.w};

    const Cov2D ch = cov2d_chain(view_point(view, mean), view, c3, a.tan_fovx, a.tan_fovy, a.h_x, a.h_y);
    const M3 J = ch.J, cov2D = ch.cov;
    // (the conic's backward and the dL_dT rows stay written out: cov2d_backward and chain_backward, the statements of K8+K9,
    //  order r before h and the rows differently, and this kernel's code follows the order -- profiles/gaussian_chain_shared_isa.md)
    const float ca = cov2D.m[0][0] + 0.3f, cb = cov2D.m[0][1], cc = cov2D.m[1][1] + 0.3f;
    const float denom = ca * cc - cb * cb;
    float dL_da = 0, dL_db = 0, dL_dc = 0;
    const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
    if (denom2inv != 0) {
      dL_da = denom2inv * (-cc * cc * dL_dcon.x + 2 * cb * cc * dL_dcon.y + (denom - ca * cc) * dL_dcon.z);
      dL_dc = denom2inv * (-ca * ca * dL_dcon.z + 2 * ca * cb * dL_dcon.y + (denom - ca * cc) * dL_dcon.x);
      dL_db = denom2inv * 2 * (cb * cc * dL_dcon.x - (denom + 2 * cb * cb) * dL_dcon.y + ca * cb * dL_dcon.z);
      if (AA) {  // r as K1 and K8+K9 compute it; on the floor h is a constant: no r-term
        const float aa_r = aa_ratio(cov2D, denom);
        if (aa_r > AA_R_FLOOR) {
          const float x = cov2D.m[0][0], y = cov2D.m[1][1], z = cb, w = 0.3f;
          const float dL_dr = acc_m2d.w * aa_ow / (2.f * aa_r);
          const float sc = dL_dr * w / (denom * denom);
          dL_da += sc * (y * y + w * y + z * z);
          dL_dc += sc * (x * x + w * x + z * z);
          dL_db += sc * (-2.f * z * (x + y + w));
        }
      }
    }
    const auto& Tm = ch.T.m;
    const auto& V = ch.Vrk.m;
    float dT0[3], dT1[3];  // dL/dT[0][r], dL/dT[1][r]: dL_dT00 .. dL_dT12 of K8
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float u0 = Tm[0][0] * V[r][0] + Tm[0][1] * V[r][1] + Tm[0][2] * V[r][2];
      const float u1 = Tm[1][0] * V[r][0] + Tm[1][1] * V[r][1] + Tm[1][2] * V[r][2];
      dT0[r] = 2 * u0 * dL_da + u1 * dL_db;
      dT1[r] = 2 * u1 * dL_dc + u0 * dL_db;
    }
    const V3 dL_dt = chain_dt(ch, dT0, dT1, a.h_x, a.h_y);
    float dt[3] = {dL_dt.x, dL_dt.y, dL_dt.z};
    if (DEPTH) dt[2] += acc_col.w;  // the depth image's share: d = t.z
    const float mu[4] = {mean.x, mean.y, mean.z, 1.f};
    // t = (mu, 1) V
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) s[c * 3 + r] += dt[r] * mu[c];
    // T = W J with W[k][r] = V[r][k]: dL/dV[r][k] = sum_c dL/dT[c][r] J[c][k] (J[0][1] = J[1][0] = 0)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      s[r * 3 + 0] += dT0[r] * J.m[0][0];
      s[r * 3 + 1] += dT1[r] * J.m[1][1];
      s[r * 3 + 2] += dT0[r] * J.m[0][2] + dT1[r] * J.m[1][2];
    }
    // p_hom = (mu, 1) PV, ndc = p_hom.xy / (p_hom.w + 1e-7)
    const HomTerms hm = hom_backward_terms(proj, mean);
    const float m_w = hm.m_w, mul1 = hm.mul1, mul2 = hm.mul2;
    const float dp[3] = {g2x * m_w, g2y * m_w, -(mul1 * g2x + mul2 * g2y)};  // columns 0, 1, 3
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) s[12 + c * 3 + r] += dp[r] * mu[c];
    // dir = mu - campos (degree 0: the colour does not depend on the direction, K1 wrote no dcol)
    if (a.sh && a.D > 0) {
      const V3 dRGBdx = *reinterpret_cast<const V3*>(a.dcol[0] + 3 * idx);
      const V3 dRGBdy = *reinterpret_cast<const V3*>(a.dcol[1] + 3 * idx);
      const V3 dRGBdz = *reinterpret_cast<const V3*>(a.dcol[2] + 3 * idx);
      const uint8_t cl = a.clamped[idx];
      const V3 dL_dRGB = unclamped_rgb_grad(V3{acc_col.x, acc_col.y, acc_col.z}, cl);
      const V3 v = {mean.x - cam.campos[0], mean.y - cam.campos[1], mean.z - cam.campos[2]};
      const V3 dv = {dot3(dRGBdx, dL_dRGB), dot3(dRGBdy, dL_dRGB), dot3(dRGBdz, dL_dRGB)};
      // dnormvdv, written out: each component is subtracted as soon as it is there, and the code follows that order
      const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
      const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
      s[24] -= ((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32;
      s[25] -= (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32;
      s[26] -= (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32;
    }
  }

  // wave (DPP) -> block (LDS) -> one row of partial sums per block, every entry written
  const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
  if (__ballot(wave_any) != 0ull) {
#pragma unroll
    for (int k = 0; k < POSE_SUMS; ++k) {
      const float v = wave_sum_to_lane63(s[k]);
      if (lane == 63) sh_part[wv][k] = v;
    }
    if (lane >= POSE_SUMS && lane < POSE_SUMS_PAD) sh_part[wv][lane] = 0.f;
  } else if (lane < POSE_SUMS_PAD) {
    sh_part[wv][lane] = 0.f;  // (the arithmetic and the reduction skipped: all 64 lanes hold zeros)
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)POSE_SUMS_PAD) {
    const int k = (int)threadIdx.x;
    a.partials[(size_t)blockIdx.x * POSE_SUMS_PAD + k] = ((sh_part[0][k] + sh_part[1][k]) + sh_part[2][k]) + sh_part[3][k];
  }
}
static_assert(GAUSS_BLOCK == 256, "pose_backward_kernel adds the partial sums of four waves");

// One workgroup: the blocks' rows in ascending order, in double -> all 35 output floats, structural zeros included.
// The sum itself is a chain of at most 1024 double adds per column, a few microseconds; what it must not wait for is a
// memory round trip per row (32 threads walking 1024 rows straight out of memory cost the backward 0.22 ms).  So all 256 threads
// bring the rows in, POSE_FIN_ROWS at a time, with coalesced 16-byte loads issued a tile ahead, and the first 32 threads add
// a tile's rows out of LDS while the next tile is in flight.
constexpr int POSE_FIN_THREADS = 256, POSE_FIN_ROWS = 256;
constexpr int POSE_FIN_F4 = POSE_FIN_ROWS * POSE_SUMS_PAD / 4 / POSE_FIN_THREADS;  // float4 per thread and tile (8)
__global__ void __launch_bounds__(POSE_FIN_THREADS) pose_finalize_kernel(int blocks, const float* __restrict__ partials,
                                                                         float* __restrict__ out) {
  __shared__ float4 tile[POSE_FIN_ROWS * POSE_SUMS_PAD / 4];  // 32 KB
  __shared__ float tot[POSE_SUMS_PAD];
  const int t = (int)threadIdx.x;
  const float4* const src = reinterpret_cast<const float4*>(partials);
  const int total4 = blocks * (POSE_SUMS_PAD / 4);
  float4 nxt[POSE_FIN_F4];
  const auto fetch = [&](int row0) {
#pragma unroll
    for (int i = 0; i < POSE_FIN_F4; ++i) {
      const int j = row0 * (POSE_SUMS_PAD / 4) + i * POSE_FIN_THREADS + t;
      nxt[i] = j < total4 ? src[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  double d = 0.0;
  fetch(0);
  for (int row0 = 0; row0 < blocks; row0 += POSE_FIN_ROWS) {
#pragma unroll
    for (int i = 0; i < POSE_FIN_F4; ++i) tile[i * POSE_FIN_THREADS + t] = nxt[i];
    __syncthreads();
    if (row0 + POSE_FIN_ROWS < blocks) fetch(row0 + POSE_FIN_ROWS);
    if (t < POSE_SUMS_PAD) {
      const float* const rows = reinterpret_cast<const float*>(tile);
      const int n = min(POSE_FIN_ROWS, blocks - row0);
      for (int r = 0; r < n; ++r) d += (double)rows[r * POSE_SUMS_PAD + t];
    }
    __syncthreads();
  }
  if (t < POSE_SUMS_PAD) tot[t] = (float)d;
  __syncthreads();
  if (t >= POSE_OUT) return;
  float v = 0.f;
  if (t < 16) {  // viewmatrix[4 c + r]: r = 3 is a structural zero
    const int c = t >> 2, r = t & 3;
    if (r < 3) v = tot[c * 3 + r];
  } else if (t < 32) {  // projmatrix[4 c + r]: r = 2 is a structural zero
    const int c = (t - 16) >> 2, r = (t - 16) & 3;
    if (r != 2) v = tot[12 + c * 3 + (r == 3 ? 2 : r)];
  } else {
    v = tot[24 + (t - 32)];
  }
  out[t] = v;
}
static_assert(POSE_FIN_F4 * POSE_FIN_THREADS * 4 == POSE_FIN_ROWS * POSE_SUMS_PAD, "a tile is a whole number of float4 per thread");

hipError_t launch_pose_backward(hipStream_t s, const PoseArgs& a, bool depth, bool antialias, float* pose_grad) {
  const int nb = pose_blocks(a.P);
  if (antialias) {
    if (depth) hipLaunchKernelGGL((pose_backward_kernel<true, true>), dim3(nb), dim3(GAUSS_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((pose_backward_kernel<false, true>), dim3(nb), dim3(GAUSS_BLOCK), 0, s, a);
  } else {
    if (depth) hipLaunchKernelGGL((pose_backward_kernel<true, false>), dim3(nb), dim3(GAUSS_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((pose_backward_kernel<false, false>), dim3(nb), dim3(GAUSS_BLOCK), 0, s, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pose_finalize_kernel, dim3(1), dim3(POSE_FIN_THREADS), 0, s, nb, a.partials, pose_grad);
  return hipGetLastError();
}

}  // namespace gsr
