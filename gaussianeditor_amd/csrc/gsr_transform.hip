// gsr_transform.hip -- similarity transforms of Gaussians, x -> s R x + t, with the rotation of the spherical-harmonic
// coefficients: gsr_sh_rotation and gsr_transform_rows of include/gsr.h, where the mathematics is
// stated.
//
// Host.  The caller's matrix is turned into a unit quaternion q_R (Shepperd's method, binary64, w >= 0) and back into the
// matrix R^ = matrix(q_R): positions, orientations and SH coefficients all see the same exactly-orthonormal rotation.  The
// SH rotation matrices D^l (l = 1..3) are defined by Y(R^ d) = D^l Y(d) for every unit d, Y the real basis of the
// rasterizer (gsr_kernels.h: SH_C1..3 and their signs).  They are built from that definition: for a fixed set of 2l+1
// directions d_i whose basis matrix A = [Y(d_1) .. Y(d_n)] is well conditioned (condition numbers 1, 1.7 and 2.2),
// D^l = [Y(R^ d_1) .. Y(R^ d_n)] A^-1, A^-1 by Gauss-Jordan elimination with partial pivoting, in binary64.  Everything travels to the
// kernel as its argument: no host-to-device copy, no workspace, no synchronisation.
//
// Kernel.  One lane per row, TR_BLOCK rows per block.  A features_rest row is 3 (rest) floats (180 bytes at SH3) at a
// 4-byte-aligned address, so the block stages its contiguous span of rows through LDS with coalesced dword loads, each lane
// transforms its own row inside LDS (row stride odd: no bank conflicts), and the span is stored back with coalesced dword
// stores PREDICATED on the row's mask: a row outside the mask is never stored to, not even with its own value.  A block
// without a selected row reads nothing.  The 83 doubles of D are staged once per block in LDS (broadcast reads).  xyz,
// rotation and scaling rows are 12 / 16 / 12 bytes: read and written by their lane directly.  Every row is evaluated in
// binary64 from the binary32 inputs and rounded once at the store (-ffp-contract=off: one IEEE operation per operator); no
// atomics: the same bits on every run.  All element offsets are 64-bit (180 row passes 2^32 at row 23 860 930).
#include <math.h>

#include "gsr_common.h"

using namespace gsr;

namespace {

constexpr int TR_BLOCK = 256;  // rows per block (gaussianeditor_amd/transform.py: ROWS_PER_BLOCK)

constexpr double TR_C1 = 0.4886025119029199;
constexpr double TR_C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                             0.5462742152960396};
constexpr double TR_C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                             -0.4570457994644658, 1.445305721320277,  -0.5900435899266435};

// the 2l+1 basis functions of band l at the unit direction d, in the order and with the signs of the rasterizer
void sh_band(int l, const double d[3], double* y) {
  const double x = d[0], yy_ = d[1], z = d[2];
  const double xx = x * x, yy = yy_ * yy_, zz = z * z, xy = x * yy_, yz = yy_ * z, xz = x * z;
  if (l == 1) {
    y[0] = -TR_C1 * yy_;
    y[1] = TR_C1 * z;
    y[2] = -TR_C1 * x;
  } else if (l == 2) {
    y[0] = TR_C2[0] * xy;
    y[1] = TR_C2[1] * yz;
    y[2] = TR_C2[2] * (2.0 * zz - xx - yy);
    y[3] = TR_C2[3] * xz;
    y[4] = TR_C2[4] * (xx - yy);
  } else {
    y[0] = TR_C3[0] * yy_ * (3.0 * xx - yy);
    y[1] = TR_C3[1] * xy * z;
    y[2] = TR_C3[2] * yy_ * (4.0 * zz - xx - yy);
    y[3] = TR_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
    y[4] = TR_C3[4] * x * (4.0 * zz - xx - yy);
    y[5] = TR_C3[5] * z * (xx - yy);
    y[6] = TR_C3[6] * x * (xx - 3.0 * yy);
  }
}

// the sample directions of each band (normalised before use)
constexpr int TR_DIRS[3][7][3] = {
    {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}},
    {{0, 2, 0}, {-2, -1, 0}, {-2, 2, 1}, {2, -1, 1}, {1, 2, 2}},
    {{2, 1, 2}, {2, 2, 0}, {2, -2, 0}, {-1, -1, 1}, {0, 2, -1}, {-2, 1, 2}, {-2, 2, -2}},
};

// inv = a^-1 for an n x n matrix (n <= 7), Gauss-Jordan with partial pivoting; false for a singular matrix
bool invert(int n, const double a[7][7], double inv[7][7]) {
  double m[7][14];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      m[i][j] = a[i][j];
      m[i][n + j] = i == j ? 1.0 : 0.0;
    }
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int i = c + 1; i < n; ++i)
      if (fabs(m[i][c]) > fabs(m[p][c])) p = i;
    if (!(fabs(m[p][c]) > 1e-12)) return false;
    if (p != c)
      for (int j = 0; j < 2 * n; ++j) {
        const double t = m[c][j];
        m[c][j] = m[p][j];
        m[p][j] = t;
      }
    const double piv = m[c][c];
    for (int j = 0; j < 2 * n; ++j) m[c][j] /= piv;
    for (int i = 0; i < n; ++i) {
      if (i == c) continue;
      const double f = m[i][c];
      if (f == 0.0) continue;
      for (int j = 0; j < 2 * n; ++j) m[i][j] -= f * m[c][j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) inv[i][j] = m[i][n + j];
  return true;
}

// what the kernel needs of the transform: by value in its argument segment
struct TrParams {
  double R[9];   // R^ = matrix(q_R), row-major
  double q[4];   // q_R (w, x, y, z), unit, w >= 0
  double t[3];
  double s, eps;
  double D[83];  // D1 (9) | D2 (25) | D3 (49), row-major
};

// rot (row-major, x' = rot x) -> q_R and R^; false unless rot is a proper rotation within 1e-4 (infinity norm of
// rot^T rot - I, determinant > 0) of finite numbers
bool rotation_of(const double rot[9], double q[4], double R[9]) {
  for (int i = 0; i < 9; ++i)
    if (!isfinite(rot[i])) return false;
  double worst = 0.0;
  for (int i = 0; i < 3; ++i) {
    double row = 0.0;
    for (int j = 0; j < 3; ++j) {
      double g = 0.0;
      for (int k = 0; k < 3; ++k) g += rot[3 * k + i] * rot[3 * k + j];
      row += fabs(g - (i == j ? 1.0 : 0.0));
    }
    worst = row > worst ? row : worst;
  }
  if (!(worst <= 1e-4)) return false;
  const double det = rot[0] * (rot[4] * rot[8] - rot[5] * rot[7]) - rot[1] * (rot[3] * rot[8] - rot[5] * rot[6]) +
                     rot[2] * (rot[3] * rot[7] - rot[4] * rot[6]);
  if (!(det > 0.0)) return false;
  // Shepperd: the largest of (trace, r00, r11, r22) decides which component is taken from a square root
  const double r00 = rot[0], r11 = rot[4], r22 = rot[8], tr = r00 + r11 + r22;
  double w, x, y, z;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    w = 1.0 + tr;
    x = rot[7] - rot[5];
    y = rot[2] - rot[6];
    z = rot[3] - rot[1];
  } else if (r00 >= r11 && r00 >= r22) {
    w = rot[7] - rot[5];
    x = 1.0 + r00 - r11 - r22;
    y = rot[1] + rot[3];
    z = rot[2] + rot[6];
  } else if (r11 >= r22) {
    w = rot[2] - rot[6];
    x = rot[1] + rot[3];
    y = 1.0 - r00 + r11 - r22;
    z = rot[5] + rot[7];
  } else {
    w = rot[3] - rot[1];
    x = rot[2] + rot[6];
    y = rot[5] + rot[7];
    z = 1.0 - r00 - r11 + r22;
  }
  const double n = sqrt(((w * w + x * x) + y * y) + z * z);
  if (!(n > 0.0)) return false;
  const double sgn = w < 0.0 ? -1.0 : 1.0;
  w = sgn * w / n;
  x = sgn * x / n;
  y = sgn * y / n;
  z = sgn * z / n;
  q[0] = w;
  q[1] = x;
  q[2] = y;
  q[3] = z;
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
  return true;
}

// D1 | D2 | D3 of the rotation R (row-major) into out[83]
bool sh_rotation_of(const double R[9], double out[83]) {
  int at = 0;
  for (int l = 1; l <= 3; ++l) {
    const int n = 2 * l + 1;
    double A[7][7], Ar[7][7], Ai[7][7];
    for (int i = 0; i < n; ++i) {
      const int* v = TR_DIRS[l - 1][i];
      const double len = sqrt((double)(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
      const double d[3] = {v[0] / len, v[1] / len, v[2] / len};
      const double rd[3] = {(R[0] * d[0] + R[1] * d[1]) + R[2] * d[2], (R[3] * d[0] + R[4] * d[1]) + R[5] * d[2],
                            (R[6] * d[0] + R[7] * d[1]) + R[8] * d[2]};
      double y[7], yr[7];
      sh_band(l, d, y);
      sh_band(l, rd, yr);
      for (int m = 0; m < n; ++m) {
        A[m][i] = y[m];
        Ar[m][i] = yr[m];
      }
    }
    if (!invert(n, A, Ai)) return false;
    // D = Ar A^-1 = I + (Ar - A) A^-1: the identity rotation gives exactly I, a small one loses nothing to cancellation
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += (Ar[i][k] - A[i][k]) * Ai[k][j];
        out[at + i * n + j] = (i == j ? 1.0 : 0.0) + acc;
      }
    at += n * n;
  }
  return true;
}

struct alignas(4) TrF3 {
  float x, y, z;
};
struct alignas(4) TrF4 {
  float w, x, y, z;
};

// floats of one features_rest row and its stride in LDS (odd: lane i's row starts in bank 45 i mod 32, all different)
template <int REST>
struct TrRow {
  static constexpr int W = 3 * REST;
  static constexpr int STRIDE = W | 1;
};

// One band of one row in LDS: c' = D c for the three channels at once.  N = 2l+1, D at sD[AT .. AT + N N), the band's
// coefficients at mine[3 (FIRST + m) + channel].  Every element of D is read once (a broadcast read) and used three times;
// each sum runs over k in ascending order.
template <int N, int AT, int FIRST>
__device__ __forceinline__ void tr_band(float* mine, const double* sD) {
  double c[N][3];
#pragma unroll
  for (int m = 0; m < N; ++m)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[m][ch] = (double)mine[3 * (FIRST + m) + ch];
#pragma unroll
  for (int m = 0; m < N; ++m) {
    const double d0 = sD[AT + N * m];
    double a0 = d0 * c[0][0], a1 = d0 * c[0][1], a2 = d0 * c[0][2];
#pragma unroll
    for (int k = 1; k < N; ++k) {
      const double d = sD[AT + N * m + k];
      a0 = a0 + d * c[k][0];
      a1 = a1 + d * c[k][1];
      a2 = a2 + d * c[k][2];
    }
    mine[3 * (FIRST + m)] = (float)a0;  // (c is in registers: the row can be overwritten as it is computed)
    mine[3 * (FIRST + m) + 1] = (float)a1;
    mine[3 * (FIRST + m) + 2] = (float)a2;
  }
}

template <int REST>
__global__ void __launch_bounds__(TR_BLOCK) transform_rows_kernel(int64_t P, float* __restrict__ xyz,
                                                                 float* __restrict__ rotation, float* __restrict__ scaling,
                                                                 float* __restrict__ sh_rest,
                                                                 const uint8_t* __restrict__ mask, const TrParams prm) {
  constexpr int W = TrRow<REST>::W, STRIDE = TrRow<REST>::STRIDE;
  __shared__ float rows[REST > 0 ? TR_BLOCK * STRIDE : 1];
  __shared__ double sD[REST > 0 ? 83 : 1];
  __shared__ uint8_t sel_sh[TR_BLOCK];
  const int64_t row0 = (int64_t)blockIdx.x * TR_BLOCK;
  const int nrows = (int)((P - row0) < (int64_t)TR_BLOCK ? (P - row0) : (int64_t)TR_BLOCK);
  const int tid = (int)threadIdx.x;
  const int64_t i = row0 + tid;
  const bool sel = tid < nrows && (mask == nullptr || mask[i] != 0);
  sel_sh[tid] = sel ? 1 : 0;
  if (__syncthreads_or(sel ? 1 : 0) == 0) return;  // (also orders sel_sh) no selected row: nothing is read or written

  if (REST > 0 && sh_rest != nullptr) {  // (uniform: the whole block takes the branch or none of it does)
    if (tid < 83) sD[tid] = prm.D[tid];
    float* const span = sh_rest + row0 * (int64_t)W;  // 64-bit element offset
    const int total = nrows * W;
    for (int e = tid; e < total; e += TR_BLOCK) {
      const int r = e / W;
      rows[r * STRIDE + (e - r * W)] = span[e];
    }
    __syncthreads();
    if (sel) {
      float* const mine = rows + tid * STRIDE;
      tr_band<3, 0, 0>(mine, sD);
      if (REST >= 8) tr_band<5, 9, 3>(mine, sD);
      if (REST >= 15) tr_band<7, 34, 8>(mine, sD);
    }
    __syncthreads();
    for (int e = tid; e < total; e += TR_BLOCK) {
      const int r = e / W;
      if (sel_sh[r] != 0) span[e] = rows[r * STRIDE + (e - r * W)];  // rows outside the mask are never stored to
    }
  }

  if (!sel) return;
  if (xyz != nullptr) {
    const TrF3 p = reinterpret_cast<const TrF3*>(xyz)[i];
    const double x = p.x, y = p.y, z = p.z;
    TrF3 o;
    o.x = (float)(prm.s * ((prm.R[0] * x + prm.R[1] * y) + prm.R[2] * z) + prm.t[0]);
    o.y = (float)(prm.s * ((prm.R[3] * x + prm.R[4] * y) + prm.R[5] * z) + prm.t[1]);
    o.z = (float)(prm.s * ((prm.R[6] * x + prm.R[7] * y) + prm.R[8] * z) + prm.t[2]);
    reinterpret_cast<TrF3*>(xyz)[i] = o;
  }
  if (rotation != nullptr) {  // q' = q_R (x) q, the Hamilton product; the raw norm is kept
    const TrF4 p = reinterpret_cast<const TrF4*>(rotation)[i];
    const double w1 = prm.q[0], x1 = prm.q[1], y1 = prm.q[2], z1 = prm.q[3];
    const double w2 = p.w, x2 = p.x, y2 = p.y, z2 = p.z;
    TrF4 o;
    o.w = (float)(((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2);
    o.x = (float)(((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2);
    o.y = (float)(((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2);
    o.z = (float)(((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2);
    reinterpret_cast<TrF4*>(rotation)[i] = o;
  }
  if (scaling != nullptr) {  // sigma' = log(exp(sigma) s + eps)
    const TrF3 p = reinterpret_cast<const TrF3*>(scaling)[i];
    TrF3 o;
    o.x = (float)log(exp((double)p.x) * prm.s + prm.eps);
    o.y = (float)log(exp((double)p.y) * prm.s + prm.eps);
    o.z = (float)log(exp((double)p.z) * prm.s + prm.eps);
    reinterpret_cast<TrF3*>(scaling)[i] = o;
  }
}

}  // namespace

extern "C" {

int gsr_sh_rotation(const double rot[9], double out[83]) {
  if (rot == nullptr || out == nullptr) return GSR_ERR_BAD_ARGUMENT;
  double q[4], R[9];
  if (!rotation_of(rot, q, R) || !sh_rotation_of(R, out)) return GSR_ERR_BAD_ARGUMENT;
  return GSR_OK;
}

int gsr_transform_rows(void* stream, int64_t P, int rest, float* xyz, float* rotation, float* scaling, float* sh_rest,
                       const uint8_t* mask, const double rot[9], const double trans[3], double scale, double scale_eps) {
  if (P < 0 || P > 0x7fffffffll) return GSR_ERR_BAD_ARGUMENT;
  if (rest != 0 && rest != 3 && rest != 8 && rest != 15) return GSR_ERR_BAD_ARGUMENT;
  if (rot == nullptr || trans == nullptr) return GSR_ERR_BAD_ARGUMENT;
  if (!(scale > 0.0) || !isfinite(scale) || !(scale_eps >= 0.0) || !isfinite(scale_eps)) return GSR_ERR_BAD_ARGUMENT;
  if (!isfinite(trans[0]) || !isfinite(trans[1]) || !isfinite(trans[2])) return GSR_ERR_BAD_ARGUMENT;
  TrParams prm;
  if (!rotation_of(rot, prm.q, prm.R)) return GSR_ERR_BAD_ARGUMENT;
  if (sh_rest != nullptr && rest == 0) return GSR_ERR_BAD_ARGUMENT;
  if (P == 0) return GSR_OK;
  if (xyz == nullptr && rotation == nullptr && scaling == nullptr && sh_rest == nullptr) return GSR_ERR_BAD_ARGUMENT;
  if ((((uintptr_t)xyz | (uintptr_t)rotation | (uintptr_t)scaling | (uintptr_t)sh_rest) & 3u) != 0) return GSR_ERR_BAD_ARGUMENT;
  for (int k = 0; k < 83; ++k) prm.D[k] = 0.0;
  if (sh_rest != nullptr && !sh_rotation_of(prm.R, prm.D)) return GSR_ERR_BAD_ARGUMENT;
  for (int k = 0; k < 3; ++k) prm.t[k] = trans[k];
  prm.s = scale;
  prm.eps = scale_eps;
  const dim3 grid((unsigned)((P + TR_BLOCK - 1) / TR_BLOCK)), block(TR_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  // (instantiated on the row length: a call without SH coefficients -- a translation, say -- carries none of the SH code)
  const int r = sh_rest != nullptr ? rest : 0;
  if (r == 0) transform_rows_kernel<0><<<grid, block, 0, s>>>(P, xyz, rotation, scaling, nullptr, mask, prm);
  else if (r == 3) transform_rows_kernel<3><<<grid, block, 0, s>>>(P, xyz, rotation, scaling, sh_rest, mask, prm);
  else if (r == 8) transform_rows_kernel<8><<<grid, block, 0, s>>>(P, xyz, rotation, scaling, sh_rest, mask, prm);
  else transform_rows_kernel<15><<<grid, block, 0, s>>>(P, xyz, rotation, scaling, sh_rest, mask, prm);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

}  // extern "C"
