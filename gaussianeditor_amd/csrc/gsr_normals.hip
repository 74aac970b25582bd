// gsr_normals.hip -- surface normals: the normal of a Gaussian (its shortest axis, turned towards the
// camera), the normal of the rendered depth image (central differences of the back-projected points) and the depth-normal
// consistency loss that ties the two together; the gsr_gaussian_normals_*, gsr_depth_normals_* and gsr_normal_loss_* entry
// points of include/gsr.h, where the mathematics is stated.
//
// Images.  A block of NR_THREADS lanes owns a tile of NR_TX x NR_TY pixels.  It stages z = depth / max(alpha, 1e-8) of the
// tile and a halo (1 pixel for the forwards, 2 for the backwards) in LDS as binary64, with 0 standing for "not a valid tap"
// (outside the image, alpha <= alpha_min, z <= 0 -- a valid z is positive), so that a tap is read from global memory once
// per block and every validity test is a comparison with 0: a pixel on the image border has a tap outside the image and is
// invalid without a test of its own, and no neighbour outside the image is ever dereferenced.
//   * forward: one normal per lane from its four taps.
//   * backward: a GATHER.  A depth pixel is the lower tap of the normal above it, the upper tap of the normal below it, the
//     right tap of the normal to its left and the left tap of the normal to its right; the lane rebuilds those (up to) four
//     normals from LDS -- the thirteen-point diamond -- and adds its four terms in that fixed order.  No atomics.
//   * loss: the forward never writes the depth-normal image; every block reduces its terms by a fixed tree into the
//     workspace and one block adds the block sums in ascending order.  The backward is the same gather with the upstream
//     gradient -dL_dloss / (H W) N read in place of an image of gradients, and it writes dL_dnormals from the lane's own
//     normal in the same launch.
// Gaussians.  One lane per row; a row's quaternion, scales and position are read as one 16 / 12 / 12 byte struct per lane
// (consecutive lanes, consecutive addresses), the camera matrix through uniform loads.  The backward recomputes the axis
// index and the sign: no saved state.
// Arithmetic: binary64 inside, binary32 in and out, rounded once at the store (-ffp-contract=off: one IEEE operation per
// operator).  Every sum has a fixed order: the same bits on every run and on every stream.
#include <math.h>

#include "gsr_common.h"

using namespace gsr;

namespace {

constexpr int NR_TX = 32, NR_TY = 8;         // pixels of a tile (gaussianeditor_amd/normals.py: TILE)
constexpr int NR_THREADS = NR_TX * NR_TY;    // one lane per pixel of the tile
constexpr int NR_ROWS = 256;                 // Gaussians per block
constexpr double NR_ALPHA_EPS = 1e-8;        // z = depth / max(alpha, NR_ALPHA_EPS)
constexpr double NR_MIN_LEN2 = 1e-30;        // a cross product shorter than this (squared) has no direction

struct NrView {
  int H, W;
  double ifx, ify, cx, cy;  // 1 / fx, 1 / fy: the ray of pixel (x, y) is ((x - cx) ifx, (y - cy) ify, 1)
  double alpha_min;
};

// z of the tile and HALO pixels around it into zt, row-major, (NR_TX + 2 HALO) wide; 0 = not a valid tap
template <int HALO>
__device__ __forceinline__ void nr_stage(double* zt, const NrView& v, const float* __restrict__ depth,
                                         const float* __restrict__ alpha) {
  constexpr int SW = NR_TX + 2 * HALO, SH = NR_TY + 2 * HALO;
  const int x0 = (int)blockIdx.x * NR_TX - HALO, y0 = (int)blockIdx.y * NR_TY - HALO;
  for (int e = (int)threadIdx.x; e < SW * SH; e += NR_THREADS) {
    const int ly = e / SW, lx = e - ly * SW;
    const int x = x0 + lx, y = y0 + ly;
    double z = 0.0;
    if (x >= 0 && x < v.W && y >= 0 && y < v.H) {
      const size_t at = (size_t)y * (size_t)v.W + (size_t)x;
      const double d = (double)depth[at];
      if (alpha != nullptr) {
        const double a = (double)alpha[at];
        const double q = d / (a > NR_ALPHA_EPS ? a : NR_ALPHA_EPS);
        if (a > v.alpha_min && q > 0.0) z = q;
      } else if (d > 0.0) {
        z = d;
      }
    }
    zt[e] = z;
  }
}

// the normal of the depth image at pixel (mx, my), whose z sits at zt[l] (row stride SW), with what its backward needs
struct NrNormal {
  double n[3];     // c / |c|
  double a[3];     // p(mx, my + 1) - p(mx, my - 1)
  double b[3];     // p(mx + 1, my) - p(mx - 1, my)
  double inv_len;  // 1 / |c|, c = a x b
};

// false: the pixel is invalid (its centre or one of its four taps is not a valid tap, or the cross product vanishes)
template <int SW>
__device__ __forceinline__ bool nr_normal(const double* zt, int l, int mx, int my, const NrView& v, NrNormal& o) {
  const double zc = zt[l], zu = zt[l - SW], zd = zt[l + SW], zl = zt[l - 1], zr = zt[l + 1];
  if (!(zc > 0.0 && zu > 0.0 && zd > 0.0 && zl > 0.0 && zr > 0.0)) return false;
  const double rx = ((double)mx - v.cx) * v.ifx, rxl = ((double)(mx - 1) - v.cx) * v.ifx, rxr = ((double)(mx + 1) - v.cx) * v.ifx;
  const double ry = ((double)my - v.cy) * v.ify, ryu = ((double)(my - 1) - v.cy) * v.ify, ryd = ((double)(my + 1) - v.cy) * v.ify;
  o.a[0] = zd * rx - zu * rx;
  o.a[1] = zd * ryd - zu * ryu;
  o.a[2] = zd - zu;
  o.b[0] = zr * rxr - zl * rxl;
  o.b[1] = zr * ry - zl * ry;
  o.b[2] = zr - zl;
  const double c0 = o.a[1] * o.b[2] - o.a[2] * o.b[1];
  const double c1 = o.a[2] * o.b[0] - o.a[0] * o.b[2];
  const double c2 = o.a[0] * o.b[1] - o.a[1] * o.b[0];
  const double len2 = (c0 * c0 + c1 * c1) + c2 * c2;
  if (!(len2 >= NR_MIN_LEN2)) return false;
  o.inv_len = 1.0 / sqrt(len2);
  o.n[0] = c0 * o.inv_len;
  o.n[1] = c1 * o.inv_len;
  o.n[2] = c2 * o.inv_len;
  return true;
}

// dL/da and dL/db of the normal at (mx, my) from the upstream gradient scale * up[:, my, mx]; false: the pixel is invalid
// (then `up` is not read: an invalid pixel may lie outside the image)
template <int SW>
__device__ __forceinline__ bool nr_normal_grad(const double* zt, int l, int mx, int my, const NrView& v,
                                               const float* __restrict__ up, double scale, double da[3], double db[3]) {
  NrNormal m;
  if (!nr_normal<SW>(zt, l, mx, my, v, m)) return false;
  const size_t plane = (size_t)v.H * (size_t)v.W, at = (size_t)my * (size_t)v.W + (size_t)mx;
  const double g0 = scale * (double)up[at], g1 = scale * (double)up[plane + at], g2 = scale * (double)up[2 * plane + at];
  const double ng = (m.n[0] * g0 + m.n[1] * g1) + m.n[2] * g2;
  // dL/dc = (g - n (n . g)) / |c|;  c = a x b: dL/da = b x dL/dc, dL/db = dL/dc x a
  const double e0 = (g0 - m.n[0] * ng) * m.inv_len, e1 = (g1 - m.n[1] * ng) * m.inv_len, e2 = (g2 - m.n[2] * ng) * m.inv_len;
  da[0] = m.b[1] * e2 - m.b[2] * e1;
  da[1] = m.b[2] * e0 - m.b[0] * e2;
  da[2] = m.b[0] * e1 - m.b[1] * e0;
  db[0] = e1 * m.a[2] - e2 * m.a[1];
  db[1] = e2 * m.a[0] - e0 * m.a[2];
  db[2] = e0 * m.a[1] - e1 * m.a[0];
  return true;
}

__global__ void __launch_bounds__(NR_THREADS)
depth_normals_forward_kernel(NrView v, const float* __restrict__ depth, const float* __restrict__ alpha, float* __restrict__ out) {
  constexpr int SW = NR_TX + 2;
  __shared__ double zt[SW * (NR_TY + 2)];
  nr_stage<1>(zt, v, depth, alpha);
  __syncthreads();
  const int lx = (int)threadIdx.x % NR_TX, ly = (int)threadIdx.x / NR_TX;
  const int x = (int)blockIdx.x * NR_TX + lx, y = (int)blockIdx.y * NR_TY + ly;
  if (x >= v.W || y >= v.H) return;
  NrNormal m;
  const bool ok = nr_normal<SW>(zt, (ly + 1) * SW + lx + 1, x, y, v, m);
  const size_t plane = (size_t)v.H * (size_t)v.W, at = (size_t)y * (size_t)v.W + (size_t)x;
  out[at] = ok ? (float)m.n[0] : 0.0f;
  out[plane + at] = ok ? (float)m.n[1] : 0.0f;
  out[2 * plane + at] = ok ? (float)m.n[2] : 0.0f;
}

// partial[block] = sum over the tile's valid pixels of A - <N, n_d>, a fixed tree
__global__ void __launch_bounds__(NR_THREADS)
normal_loss_forward_kernel(NrView v, const float* __restrict__ normals, const float* __restrict__ depth,
                           const float* __restrict__ alpha, double* __restrict__ partial) {
  constexpr int SW = NR_TX + 2;
  __shared__ double zt[SW * (NR_TY + 2)];
  __shared__ double red[NR_THREADS];
  nr_stage<1>(zt, v, depth, alpha);
  __syncthreads();
  const int lx = (int)threadIdx.x % NR_TX, ly = (int)threadIdx.x / NR_TX;
  const int x = (int)blockIdx.x * NR_TX + lx, y = (int)blockIdx.y * NR_TY + ly;
  double t = 0.0;
  NrNormal m;
  if (x < v.W && y < v.H && nr_normal<SW>(zt, (ly + 1) * SW + lx + 1, x, y, v, m)) {
    const size_t plane = (size_t)v.H * (size_t)v.W, at = (size_t)y * (size_t)v.W + (size_t)x;
    const double dot = ((double)normals[at] * m.n[0] + (double)normals[plane + at] * m.n[1]) + (double)normals[2 * plane + at] * m.n[2];
    t = (double)alpha[at] - dot;
  }
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = NR_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// out_loss = (sum of the block sums, lane t the slots t, t + 256, ... ascending, then a fixed tree) / (H W)
__global__ void __launch_bounds__(NR_THREADS)
normal_loss_finish_kernel(const double* __restrict__ partial, int64_t n, double inv_pixels, float* __restrict__ out_loss) {
  __shared__ double red[NR_THREADS];
  double t = 0.0;
  for (int64_t i = (int64_t)threadIdx.x; i < n; i += NR_THREADS) t += partial[i];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = NR_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out_loss[0] = (float)(red[0] * inv_pixels);
}

// The backward of the depth normals (LOSS = false: the upstream gradient is the image `up` = dL_dout) and of the loss
// (LOSS = true: it is -dL_dloss / (H W) N with `up` = N, and dL_dnormals = -dL_dloss / (H W) n_d is written as well).
// Any of d_normals, d_depth, d_alpha may be NULL; d_alpha only with alpha.
template <bool LOSS>
__global__ void __launch_bounds__(NR_THREADS)
normals_backward_kernel(NrView v, const float* __restrict__ depth, const float* __restrict__ alpha, const float* __restrict__ up,
                        const float* __restrict__ dL_dloss, float* __restrict__ d_normals, float* __restrict__ d_depth,
                        float* __restrict__ d_alpha) {
  constexpr int SW = NR_TX + 4;
  __shared__ double zt[SW * (NR_TY + 4)];
  nr_stage<2>(zt, v, depth, alpha);
  __syncthreads();
  const int lx = (int)threadIdx.x % NR_TX, ly = (int)threadIdx.x / NR_TX;
  const int x = (int)blockIdx.x * NR_TX + lx, y = (int)blockIdx.y * NR_TY + ly;
  if (x >= v.W || y >= v.H) return;
  const int l = (ly + 2) * SW + lx + 2;
  const size_t plane = (size_t)v.H * (size_t)v.W, at = (size_t)y * (size_t)v.W + (size_t)x;
  const double scale = LOSS ? -(double)dL_dloss[0] / ((double)v.H * (double)v.W) : 1.0;
  if (LOSS && d_normals != nullptr) {
    NrNormal m;
    const bool ok = nr_normal<SW>(zt, l, x, y, v, m);
    d_normals[at] = ok ? (float)(scale * m.n[0]) : 0.0f;
    d_normals[plane + at] = ok ? (float)(scale * m.n[1]) : 0.0f;
    d_normals[2 * plane + at] = ok ? (float)(scale * m.n[2]) : 0.0f;
  }
  if (d_depth == nullptr && d_alpha == nullptr) return;
  double dz = 0.0;
  if (zt[l] > 0.0) {  // (a pixel that is no valid tap invalidates all four normals around it)
    const double rx = ((double)x - v.cx) * v.ifx, ry = ((double)y - v.cy) * v.ify;
    double da[3], db[3];
    // the normal above: this pixel is its lower tap, p(mx, my + 1) of a
    if (nr_normal_grad<SW>(zt, l - SW, x, y - 1, v, up, scale, da, db)) dz = dz + ((rx * da[0] + ry * da[1]) + da[2]);
    // the normal below: its upper tap, -p(mx, my - 1) of a
    if (nr_normal_grad<SW>(zt, l + SW, x, y + 1, v, up, scale, da, db)) dz = dz - ((rx * da[0] + ry * da[1]) + da[2]);
    // the normal to the left: its right tap, p(mx + 1, my) of b
    if (nr_normal_grad<SW>(zt, l - 1, x - 1, y, v, up, scale, da, db)) dz = dz + ((rx * db[0] + ry * db[1]) + db[2]);
    // the normal to the right: its left tap, -p(mx - 1, my) of b
    if (nr_normal_grad<SW>(zt, l + 1, x + 1, y, v, up, scale, da, db)) dz = dz - ((rx * db[0] + ry * db[1]) + db[2]);
  }
  if (dz == 0.0) {  // (exact zeros, never -0)
    if (d_depth != nullptr) d_depth[at] = 0.0f;
    if (d_alpha != nullptr) d_alpha[at] = 0.0f;
    return;
  }
  if (alpha == nullptr) {
    if (d_depth != nullptr) d_depth[at] = (float)dz;
    return;
  }
  // z = depth / max(alpha, eps); a valid tap has alpha > alpha_min, which may lie below eps: the clamp then has no slope
  const double a = (double)alpha[at], am = a > NR_ALPHA_EPS ? a : NR_ALPHA_EPS;
  if (d_depth != nullptr) d_depth[at] = (float)(dz / am);
  if (d_alpha != nullptr) d_alpha[at] = a > NR_ALPHA_EPS ? (float)(-(dz * (double)depth[at]) / (am * am)) : 0.0f;
}

struct alignas(4) NrF3 {
  float x, y, z;
};
struct alignas(4) NrF4 {
  float w, x, y, z;
};

// BACKWARD = false: out (P,3) = the camera-space normal of every row.  BACKWARD = true: out (P,4) = dL/drotations from
// dL_dout (P,3); the axis index and the sign are recomputed.
template <bool BACKWARD>
__global__ void __launch_bounds__(NR_ROWS)
gaussian_normals_kernel(int64_t P, const float* __restrict__ rotations, const float* __restrict__ scales,
                        const float* __restrict__ means3D, const float* __restrict__ viewmatrix,
                        const float* __restrict__ dL_dout, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NR_ROWS + threadIdx.x;
  if (i >= P) return;
  double V[12];  // V[3 r + c] = viewmatrix[r][c], r = 0..3 (row 3: the translation), c = 0..2: p_c = p_w V[:3,:3] + V[3,:3]
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[3 * r + c] = (double)viewmatrix[4 * r + c];
  const NrF4 q4 = reinterpret_cast<const NrF4*>(rotations)[i];
  const NrF3 s3 = reinterpret_cast<const NrF3*>(scales)[i];
  const NrF3 p3 = reinterpret_cast<const NrF3*>(means3D)[i];
  int k = 0;  // the shortest axis; on a tie the lowest index
  float smin = s3.x;
  if (s3.y < smin) {
    k = 1;
    smin = s3.y;
  }
  if (s3.z < smin) k = 2;
  const double qw = q4.w, qx = q4.x, qy = q4.y, qz = q4.z;
  const double inv = 1.0 / sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  const double r = qw * inv, x = qx * inv, y = qy * inv, z = qz * inv;
  double nw[3];  // column k of R(q^)
  if (k == 0) {
    nw[0] = 1.0 - 2.0 * (y * y + z * z);
    nw[1] = 2.0 * (x * y + r * z);
    nw[2] = 2.0 * (x * z - r * y);
  } else if (k == 1) {
    nw[0] = 2.0 * (x * y - r * z);
    nw[1] = 1.0 - 2.0 * (x * x + z * z);
    nw[2] = 2.0 * (y * z + r * x);
  } else {
    nw[0] = 2.0 * (x * z + r * y);
    nw[1] = 2.0 * (y * z - r * x);
    nw[2] = 1.0 - 2.0 * (x * x + y * y);
  }
  double nc[3], pc[3];
  const double px = p3.x, py = p3.y, pz = p3.z;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    nc[c] = (nw[0] * V[c] + nw[1] * V[3 + c]) + nw[2] * V[6 + c];
    pc[c] = ((px * V[c] + py * V[3 + c]) + pz * V[6 + c]) + V[9 + c];
  }
  const double sgn = ((nc[0] * pc[0] + nc[1] * pc[1]) + nc[2] * pc[2]) > 0.0 ? -1.0 : 1.0;
  if (!BACKWARD) {
    NrF3 o;
    o.x = (float)(sgn * nc[0]);
    o.y = (float)(sgn * nc[1]);
    o.z = (float)(sgn * nc[2]);
    reinterpret_cast<NrF3*>(out)[i] = o;
    return;
  }
  const NrF3 u3 = reinterpret_cast<const NrF3*>(dL_dout)[i];
  const double u[3] = {sgn * (double)u3.x, sgn * (double)u3.y, sgn * (double)u3.z};
  double g[3];  // dL/dn_w
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = (V[3 * a] * u[0] + V[3 * a + 1] * u[1]) + V[3 * a + 2] * u[2];
  double hr, hx, hy, hz;  // dL/dq^ through column k
  if (k == 0) {
    hr = 2.0 * (z * g[1] - y * g[2]);
    hx = 2.0 * (y * g[1] + z * g[2]);
    hy = 2.0 * ((x * g[1] - r * g[2]) - 2.0 * y * g[0]);
    hz = 2.0 * ((r * g[1] + x * g[2]) - 2.0 * z * g[0]);
  } else if (k == 1) {
    hr = 2.0 * (x * g[2] - z * g[0]);
    hx = 2.0 * ((y * g[0] + r * g[2]) - 2.0 * x * g[1]);
    hy = 2.0 * (x * g[0] + z * g[2]);
    hz = 2.0 * ((y * g[2] - r * g[0]) - 2.0 * z * g[1]);
  } else {
    hr = 2.0 * (y * g[0] - x * g[1]);
    hx = 2.0 * ((z * g[0] - r * g[1]) - 2.0 * x * g[2]);
    hy = 2.0 * ((r * g[0] + z * g[1]) - 2.0 * y * g[2]);
    hz = 2.0 * (x * g[0] + y * g[1]);
  }
  // through q^ = q / |q|: dL/dq = (h - q^ (q^ . h)) / |q|, orthogonal to q
  const double qh = ((r * hr + x * hx) + y * hy) + z * hz;
  NrF4 o;
  o.w = (float)((hr - r * qh) * inv);
  o.x = (float)((hx - x * qh) * inv);
  o.y = (float)((hy - y * qh) * inv);
  o.z = (float)((hz - z * qh) * inv);
  reinterpret_cast<NrF4*>(out)[i] = o;
}

// H, W >= 1 with H W and the tile grid in range; fx, fy finite and positive; cx, cy, alpha_min finite
bool nr_view(int H, int W, double fx, double fy, double cx, double cy, double alpha_min, NrView* v, dim3* grid) {
  if (H < 1 || W < 1 || (int64_t)H * (int64_t)W > 0x7fffffffll) return false;
  if (!(fx > 0.0) || !(fy > 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy) || !isfinite(alpha_min))
    return false;
  const int gx = (W + NR_TX - 1) / NR_TX, gy = (H + NR_TY - 1) / NR_TY;
  if (gy > 65535) return false;
  v->H = H;
  v->W = W;
  v->ifx = 1.0 / fx;
  v->ify = 1.0 / fy;
  v->cx = cx;
  v->cy = cy;
  v->alpha_min = alpha_min;
  *grid = dim3((unsigned)gx, (unsigned)gy);
  return true;
}

bool nr_rows_ok(int64_t P, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f) {
  if (P < 0 || P > 0x7fffffffll) return false;
  if (P == 0) return true;
  if (a == nullptr || b == nullptr || c == nullptr || d == nullptr || e == nullptr || f == nullptr) return false;
  return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f) & 3u) == 0);
}

}  // namespace

extern "C" {

int gsr_gaussian_normals_forward(void* stream, int64_t P, const float* rotations, const float* scales, const float* means3D,
                                 const float* viewmatrix, float* out) {
  if (!nr_rows_ok(P, rotations, scales, means3D, viewmatrix, out, out)) return GSR_ERR_BAD_ARGUMENT;
  if (P == 0) return GSR_OK;
  const dim3 grid((unsigned)((P + NR_ROWS - 1) / NR_ROWS)), block(NR_ROWS);
  gaussian_normals_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(P, rotations, scales, means3D, viewmatrix, nullptr, out);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_gaussian_normals_backward(void* stream, int64_t P, const float* rotations, const float* scales, const float* means3D,
                                  const float* viewmatrix, const float* dL_dout, float* dL_drotations) {
  if (!nr_rows_ok(P, rotations, scales, means3D, viewmatrix, dL_dout, dL_drotations)) return GSR_ERR_BAD_ARGUMENT;
  if (P == 0) return GSR_OK;
  const dim3 grid((unsigned)((P + NR_ROWS - 1) / NR_ROWS)), block(NR_ROWS);
  gaussian_normals_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(P, rotations, scales, means3D, viewmatrix, dL_dout,
                                                                        dL_drotations);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_depth_normals_forward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                              const float* depth, const float* alpha, float* out) {
  NrView v;
  dim3 grid;
  if (!nr_view(H, W, fx, fy, cx, cy, alpha_min, &v, &grid) || depth == nullptr || out == nullptr) return GSR_ERR_BAD_ARGUMENT;
  depth_normals_forward_kernel<<<grid, dim3(NR_THREADS), 0, (hipStream_t)stream>>>(v, depth, alpha, out);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_depth_normals_backward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                               const float* depth, const float* alpha, const float* dL_dout, float* dL_ddepth, float* dL_dalpha) {
  NrView v;
  dim3 grid;
  if (!nr_view(H, W, fx, fy, cx, cy, alpha_min, &v, &grid) || depth == nullptr || dL_dout == nullptr) return GSR_ERR_BAD_ARGUMENT;
  if (dL_dalpha != nullptr && alpha == nullptr) return GSR_ERR_BAD_ARGUMENT;
  if (dL_ddepth == nullptr && dL_dalpha == nullptr) return GSR_OK;
  normals_backward_kernel<false><<<grid, dim3(NR_THREADS), 0, (hipStream_t)stream>>>(v, depth, alpha, dL_dout, nullptr, nullptr,
                                                                                     dL_ddepth, dL_dalpha);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_normal_loss_workspace_size(int H, int W, size_t* bytes) {
  NrView v;
  dim3 grid;
  if (bytes == nullptr || !nr_view(H, W, 1.0, 1.0, 0.0, 0.0, 0.0, &v, &grid)) return GSR_ERR_BAD_ARGUMENT;
  *bytes = (size_t)grid.x * (size_t)grid.y * sizeof(double);
  return GSR_OK;
}

int gsr_normal_loss_forward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                            const float* normals, const float* depth, const float* alpha, void* workspace, float* out_loss) {
  NrView v;
  dim3 grid;
  if (!nr_view(H, W, fx, fy, cx, cy, alpha_min, &v, &grid) || normals == nullptr || depth == nullptr || alpha == nullptr ||
      workspace == nullptr || ((uintptr_t)workspace & 7u) != 0 || out_loss == nullptr)
    return GSR_ERR_BAD_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  normal_loss_forward_kernel<<<grid, dim3(NR_THREADS), 0, s>>>(v, normals, depth, alpha, (double*)workspace);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  normal_loss_finish_kernel<<<dim3(1), dim3(NR_THREADS), 0, s>>>((const double*)workspace, (int64_t)grid.x * (int64_t)grid.y,
                                                                  1.0 / ((double)H * (double)W), out_loss);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_normal_loss_backward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                             const float* normals, const float* depth, const float* alpha, const float* dL_dloss,
                             float* dL_dnormals, float* dL_ddepth, float* dL_dalpha) {
  NrView v;
  dim3 grid;
  if (!nr_view(H, W, fx, fy, cx, cy, alpha_min, &v, &grid) || normals == nullptr || depth == nullptr || alpha == nullptr ||
      dL_dloss == nullptr)
    return GSR_ERR_BAD_ARGUMENT;
  if (dL_dnormals == nullptr && dL_ddepth == nullptr && dL_dalpha == nullptr) return GSR_OK;
  normals_backward_kernel<true><<<grid, dim3(NR_THREADS), 0, (hipStream_t)stream>>>(v, depth, alpha, normals, dL_dloss, dL_dnormals,
                                                                                    dL_ddepth, dL_dalpha);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

}  // extern "C"
