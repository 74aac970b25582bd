// gsr_loss.hip -- the fused photometric loss w_l1 * L1 + w_ssim * SSIM + c of two images and its gradient (DESIGN.md
// section 15): gsr_loss_workspace_size, gsr_photometric_loss_forward, gsr_photometric_loss_backward of include/gsr.h.
//
// SSIM as 3DGS trainers evaluate it: an 11-tap Gaussian window (sigma 1.5, normalised), applied separably with zero
// padding; K(.) = "convolve with the window":
//   mu1 = K(x), mu2 = K(y), s1 = K(x^2) - mu1^2, s2 = K(y^2) - mu2^2, s12 = K(xy) - mu1 mu2, C1 = 1e-4, C2 = 9e-4,
//   A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s1 + s2 + C2, m = A1 A2 / (B1 B2), SSIM = mean(m).
// Gradient by x through three per-pixel maps the forward leaves behind,
//   dm_dmu1 = 2 mu2 A2 / (B1 B2) - 2 mu1 m / B1,  dm_ds1 = -m / B2,  dm_ds12 = 2 A1 / (B1 B2),
//   Dmu = dm_dmu1 - 2 mu1 dm_ds1 - mu2 dm_ds12,
//   dSSIM/dx = [K(Dmu) + 2 x K(dm_ds1) + y K(dm_ds12)] / N      (the window is symmetric: its adjoint is itself),
// and dL1/dx = sign(x - y) / N with sign(0) = 0.
//
// Kernel A (loss_forward_kernel): one 256-thread workgroup per 16 x 64 tile of one plane.  x and y with a 5-pixel halo go
// to LDS, a horizontal pass leaves the five row-filtered quantities in LDS, a vertical pass and the pixel maths follow in
// registers; the workgroup's sums of m and |x - y| go to ITS slot of the workspace.  loss_finish_kernel adds the slots in
// a fixed order (binary64).  Kernel B (loss_backward_kernel): the same two passes over the three maps.  No atomics: the
// loss and the gradient are the same bits on every run.
#include "../gsr_common.h"

using namespace gsr;

namespace {

constexpr int LT_W = 64, LT_H = 16;       // output pixels per workgroup
constexpr int LHALO = 5, LTAPS = 11;
constexpr int LIN_W = LT_W + 2 * LHALO;   // 74 staged columns (even: the horizontal pass reads aligned float2s)
constexpr int LIN_H = LT_H + 2 * LHALO;   // 26 staged rows
constexpr int LTHREADS = 256;
constexpr int LROWS = LT_H / (LTHREADS / LT_W);  // 4 output rows per thread, in one column
static_assert(LTHREADS % LT_W == 0 && LT_H % (LTHREADS / LT_W) == 0 && LIN_W % 2 == 0 && LT_W % 2 == 0, "tile shape");

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, evaluated in binary64 and rounded once; g[10 - i] = g[i]
__device__ __forceinline__ float tap(int i) {
  constexpr float G[6] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c40p-3f, 0x1.106560p-2f};
  return G[i <= 5 ? i : 10 - i];
}

struct TilePos {
  int plane, y0, x0;
  size_t base;  // offset of the plane
};
__device__ __forceinline__ TilePos tile_pos(int H, int W, int tiles_x, int tiles_y) {
  const unsigned b = blockIdx.x, per_plane = (unsigned)tiles_x * (unsigned)tiles_y;
  const unsigned plane = b / per_plane, t = b - plane * per_plane, ty = t / (unsigned)tiles_x, tx = t - ty * (unsigned)tiles_x;
  TilePos p;
  p.plane = (int)plane;
  p.y0 = (int)ty * LT_H;
  p.x0 = (int)tx * LT_W;
  p.base = (size_t)plane * (size_t)H * (size_t)W;
  return p;
}

// the tile of `src` with its halo -> dst[LIN_H][LIN_W]; zero outside the image (conv2d's zero padding)
__device__ __forceinline__ void stage_tile(float (*dst)[LIN_W], const float* __restrict__ src, const TilePos& p, int H, int W) {
  for (int i = (int)threadIdx.x; i < LIN_H * LIN_W; i += LTHREADS) {
    const int r = i / LIN_W, c = i - r * LIN_W;
    const int gy = p.y0 + r - LHALO, gx = p.x0 + c - LHALO;
    float v = 0.0f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = src[p.base + (size_t)gy * (size_t)W + (size_t)gx];
    dst[r][c] = v;
  }
}

// vertical pass: out[k] = sum_t g[t] col[(k + t) * LT_W], k = 0 .. LROWS - 1 (14 LDS reads for 4 outputs)
__device__ __forceinline__ void vpass(const float* col, float out[LROWS]) {
  float v[LROWS + LTAPS - 1];
#pragma unroll
  for (int i = 0; i < LROWS + LTAPS - 1; ++i) v[i] = col[i * LT_W];
#pragma unroll
  for (int k = 0; k < LROWS; ++k) {
    float a = 0.0f;
#pragma unroll
    for (int t = 0; t < LTAPS; ++t) a = __builtin_fmaf(tap(t), v[k + t], a);
    out[k] = a;
  }
}

// Sum of one value per thread over the workgroup, in a fixed order: xor butterflies inside each wave, then the four wave
// sums left to right.  Valid in every thread.
__device__ __forceinline__ float block_sum(float v, float* smem /* LTHREADS / 64 */) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();  // (smem may still be read from an earlier call)
  if (lane_id() == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = smem[0];
#pragma unroll
  for (int w = 1; w < LTHREADS / 64; ++w) s += smem[w];
  return s;
}

// Kernel A.  maps == null: the metric path (no backward follows).  w_ssim == 0 (uniform): the L1 branch -- no LDS tile,
// no convolution, the slot's SSIM sum is 0.  Both branches sum |x - y| with the same pixel -> thread mapping and the same
// reduction, so the L1 term is the same bits either way.
__global__ void __launch_bounds__(LTHREADS)
loss_forward_kernel(int H, int W, int tiles_x, int tiles_y, const float* __restrict__ img, const float* __restrict__ gt,
                    int with_ssim, float* __restrict__ maps, size_t N, float2* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float sX[LIN_H][LIN_W];
  __shared__ __attribute__((aligned(16))) float sY[LIN_H][LIN_W];
  __shared__ __attribute__((aligned(16))) float sHz[5][LIN_H][LT_W];
  __shared__ float sred[LTHREADS / 64];
  const TilePos p = tile_pos(H, W, tiles_x, tiles_y);
  const int c = (int)threadIdx.x % LT_W, rg = (int)threadIdx.x / LT_W;
  const int gx = p.x0 + c;
  float sum_m = 0.0f, sum_l1 = 0.0f;

  if (!with_ssim) {
#pragma unroll
    for (int k = 0; k < LROWS; ++k) {
      const int gy = p.y0 + rg * LROWS + k;
      if (gy < H && gx < W) {
        const size_t o = p.base + (size_t)gy * (size_t)W + (size_t)gx;
        sum_l1 += fabsf(img[o] - gt[o]);
      }
    }
  } else {
    stage_tile(sX, img, p, H, W);
    stage_tile(sY, gt, p, H, W);
    __syncthreads();
    // horizontal pass: an item = two neighbouring outputs of one staged row; a half-wave covers one row with consecutive
    // float2s (ds_read_b64 / ds_write_b64, conflict-free)
    for (int i = (int)threadIdx.x; i < LIN_H * (LT_W / 2); i += LTHREADS) {
      const int r = i / (LT_W / 2), j = i - r * (LT_W / 2);
      float x[LTAPS + 1], y[LTAPS + 1];
#pragma unroll
      for (int q = 0; q < (LTAPS + 1) / 2; ++q) {
        const float2 a = *(const float2*)&sX[r][2 * j + 2 * q], b = *(const float2*)&sY[r][2 * j + 2 * q];
        x[2 * q] = a.x; x[2 * q + 1] = a.y;
        y[2 * q] = b.x; y[2 * q + 1] = b.y;
      }
      float hx[2] = {0.0f, 0.0f}, hy[2] = {0.0f, 0.0f}, hxx[2] = {0.0f, 0.0f}, hyy[2] = {0.0f, 0.0f}, hxy[2] = {0.0f, 0.0f};
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int t = 0; t < LTAPS; ++t) {
          const float g = tap(t), xv = x[o + t], yv = y[o + t];
          const float gxv = g * xv, gyv = g * yv;
          hx[o] = __builtin_fmaf(g, xv, hx[o]);
          hy[o] = __builtin_fmaf(g, yv, hy[o]);
          hxx[o] = __builtin_fmaf(gxv, xv, hxx[o]);
          hyy[o] = __builtin_fmaf(gyv, yv, hyy[o]);
          hxy[o] = __builtin_fmaf(gxv, yv, hxy[o]);
        }
      *(float2*)&sHz[0][r][2 * j] = make_float2(hx[0], hx[1]);
      *(float2*)&sHz[1][r][2 * j] = make_float2(hy[0], hy[1]);
      *(float2*)&sHz[2][r][2 * j] = make_float2(hxx[0], hxx[1]);
      *(float2*)&sHz[3][r][2 * j] = make_float2(hyy[0], hyy[1]);
      *(float2*)&sHz[4][r][2 * j] = make_float2(hxy[0], hxy[1]);
    }
    __syncthreads();
    float mu1[LROWS], mu2[LROWS], exx[LROWS], eyy[LROWS], exy[LROWS];
    vpass(&sHz[0][rg * LROWS][c], mu1);
    vpass(&sHz[1][rg * LROWS][c], mu2);
    vpass(&sHz[2][rg * LROWS][c], exx);
    vpass(&sHz[3][rg * LROWS][c], eyy);
    vpass(&sHz[4][rg * LROWS][c], exy);
    constexpr float C1 = 1e-4f, C2 = 9e-4f;
#pragma unroll
    for (int k = 0; k < LROWS; ++k) {
      const int ly = rg * LROWS + k, gy = p.y0 + ly;
      if (gy < H && gx < W) {
        const float m1 = mu1[k], m2 = mu2[k];
        const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const float s1 = exx[k] - m11, s2 = eyy[k] - m22, s12 = exy[k] - m12;
        const float A1 = 2.0f * m12 + C1, A2 = 2.0f * s12 + C2, B1 = m11 + m22 + C1, B2 = s1 + s2 + C2;
        const float rB1 = 1.0f / B1, rB2 = 1.0f / B2;
        const float m = (A1 * rB1) * (A2 * rB2);
        sum_m += m;
        sum_l1 += fabsf(sX[ly + LHALO][c + LHALO] - sY[ly + LHALO][c + LHALO]);
        if (maps != nullptr) {
          const float rBB = rB1 * rB2;
          const float dm_dmu1 = 2.0f * m2 * A2 * rBB - 2.0f * m1 * m * rB1;
          const float dm_ds1 = -(m * rB2);
          const float dm_ds12 = 2.0f * A1 * rBB;
          const float Dmu = dm_dmu1 - 2.0f * m1 * dm_ds1 - m2 * dm_ds12;
          const size_t o = p.base + (size_t)gy * (size_t)W + (size_t)gx;
          maps[o] = Dmu;
          maps[N + o] = dm_ds1;
          maps[2 * N + o] = dm_ds12;
        }
      }
    }
  }
  const float tm = block_sum(sum_m, sred), tl = block_sum(sum_l1, sred);
  if (threadIdx.x == 0) partial[blockIdx.x] = make_float2(tm, tl);
}

// out3 = (loss, l1, ssim): the slots added in binary64, thread t the slots t, t + 256, ... in ascending order, then a
// fixed tree.  Without the SSIM branch out3[2] is NaN ("not evaluated") and the term is left out of the loss.
__global__ void __launch_bounds__(LTHREADS)
loss_finish_kernel(const float2* __restrict__ partial, int n, double inv_n, float w_l1, float w_ssim, float c, int with_ssim,
                   float* __restrict__ out3) {
  __shared__ double sm[LTHREADS], sl[LTHREADS];
  double am = 0.0, al = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += LTHREADS) {
    const float2 v = partial[i];
    am += (double)v.x;
    al += (double)v.y;
  }
  sm[threadIdx.x] = am;
  sl[threadIdx.x] = al;
  __syncthreads();
  for (int d = LTHREADS / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      sm[threadIdx.x] += sm[threadIdx.x + d];
      sl[threadIdx.x] += sl[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double l1 = sl[0] * inv_n, ssim = sm[0] * inv_n;
    const double loss = (double)w_l1 * l1 + (with_ssim ? (double)w_ssim * ssim : 0.0) + (double)c;
    out3[0] = (float)loss;
    out3[1] = (float)l1;
    out3[2] = with_ssim ? (float)ssim : __builtin_nanf("");
  }
}

// Kernel B.  dL_dimg = g * (ws_n * [K(Dmu) + 2 x K(dm_ds1) + y K(dm_ds12)] + wl_n * sign(x - y)), g = *dL_dloss read on the
// device, ws_n = w_ssim / N, wl_n = w_l1 / N.  The bracket does not depend on g: scaling the loss scales the gradient by
// one rounding.  with_ssim == 0 (uniform): the maps are not read.
__global__ void __launch_bounds__(LTHREADS)
loss_backward_kernel(int H, int W, int tiles_x, int tiles_y, const float* __restrict__ img, const float* __restrict__ gt,
                     const float* __restrict__ maps, size_t N, int with_ssim, float ws_n, float wl_n,
                     const float* __restrict__ dL_dloss, float* __restrict__ dL_dimg) {
  __shared__ __attribute__((aligned(16))) float sM[3][LIN_H][LIN_W];
  __shared__ __attribute__((aligned(16))) float sHz[3][LIN_H][LT_W];
  const TilePos p = tile_pos(H, W, tiles_x, tiles_y);
  const int c = (int)threadIdx.x % LT_W, rg = (int)threadIdx.x / LT_W;
  const int gx = p.x0 + c;
  const float g = dL_dloss[0];
  float k0[LROWS] = {}, k1[LROWS] = {}, k2[LROWS] = {};
  if (with_ssim) {
    stage_tile(sM[0], maps, p, H, W);
    stage_tile(sM[1], maps + N, p, H, W);
    stage_tile(sM[2], maps + 2 * N, p, H, W);
    __syncthreads();
    for (int i = (int)threadIdx.x; i < LIN_H * (LT_W / 2); i += LTHREADS) {
      const int r = i / (LT_W / 2), j = i - r * (LT_W / 2);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        float v[LTAPS + 1];
#pragma unroll
        for (int u = 0; u < (LTAPS + 1) / 2; ++u) {
          const float2 a = *(const float2*)&sM[q][r][2 * j + 2 * u];
          v[2 * u] = a.x; v[2 * u + 1] = a.y;
        }
        float h0 = 0.0f, h1 = 0.0f;
#pragma unroll
        for (int t = 0; t < LTAPS; ++t) {
          h0 = __builtin_fmaf(tap(t), v[t], h0);
          h1 = __builtin_fmaf(tap(t), v[t + 1], h1);
        }
        *(float2*)&sHz[q][r][2 * j] = make_float2(h0, h1);
      }
    }
    __syncthreads();
    vpass(&sHz[0][rg * LROWS][c], k0);
    vpass(&sHz[1][rg * LROWS][c], k1);
    vpass(&sHz[2][rg * LROWS][c], k2);
  }
#pragma unroll
  for (int k = 0; k < LROWS; ++k) {
    const int gy = p.y0 + rg * LROWS + k;
    if (gy < H && gx < W) {
      const size_t o = p.base + (size_t)gy * (size_t)W + (size_t)gx;
      const float x = img[o], y = gt[o], d = x - y;
      const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
      float v = wl_n * sgn;
      if (with_ssim) {
        const float br = __builtin_fmaf(y, k2[k], __builtin_fmaf(2.0f * x, k1[k], k0[k]));
        v = __builtin_fmaf(ws_n, br, v);
      }
      dL_dimg[o] = g * v;
    }
  }
}

struct LossGrid {
  int tiles_x, tiles_y;
  int64_t blocks;
  size_t N;
};
// false: a size is not positive, or there are more than 2^40 pixels / 2^24 - 1 tiles
bool loss_grid(int planes, int H, int W, LossGrid* g) {
  if (planes <= 0 || H <= 0 || W <= 0) return false;
  g->tiles_x = (W + LT_W - 1) / LT_W;
  g->tiles_y = (H + LT_H - 1) / LT_H;
  g->blocks = (int64_t)planes * g->tiles_x * g->tiles_y;
  const int64_t hw = (int64_t)H * W;
  if (hw > ((int64_t)1 << 40) / planes) return false;
  g->N = (size_t)(hw * planes);
  return g->blocks <= 0xffffff;  // (blocks * 256 threads stays below 2^32)
}

}  // namespace

extern "C" {

int gsr_loss_workspace_size(int planes, int H, int W, size_t* bytes) {
  LossGrid g;
  if (bytes == nullptr || !loss_grid(planes, H, W, &g)) return GSR_ERR_BAD_ARGUMENT;
  *bytes = align_up(sizeof(float2) * (size_t)g.blocks);
  return GSR_OK;
}

int gsr_photometric_loss_forward(void* stream, int planes, int H, int W, const float* img, const float* gt, float w_l1,
                                 float w_ssim, float c, float* maps, void* workspace, float* out3) {
  LossGrid g;
  if (img == nullptr || gt == nullptr || workspace == nullptr || out3 == nullptr || !loss_grid(planes, H, W, &g))
    return GSR_ERR_BAD_ARGUMENT;
  if (((uintptr_t)workspace & 7u) != 0) return GSR_ERR_BAD_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  const int with_ssim = w_ssim != 0.0f;
  loss_forward_kernel<<<dim3((unsigned)g.blocks), dim3(LTHREADS), 0, s>>>(H, W, g.tiles_x, g.tiles_y, img, gt, with_ssim,
                                                                         with_ssim ? maps : nullptr, g.N, (float2*)workspace);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  loss_finish_kernel<<<dim3(1), dim3(LTHREADS), 0, s>>>((const float2*)workspace, (int)g.blocks, 1.0 / (double)g.N, w_l1,
                                                       w_ssim, c, with_ssim, out3);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_photometric_loss_backward(void* stream, int planes, int H, int W, const float* img, const float* gt,
                                  const float* maps, float w_l1, float w_ssim, const float* dL_dloss, float* dL_dimg) {
  LossGrid g;
  if (img == nullptr || gt == nullptr || maps == nullptr || dL_dloss == nullptr || dL_dimg == nullptr ||
      !loss_grid(planes, H, W, &g))
    return GSR_ERR_BAD_ARGUMENT;
  const double inv_n = 1.0 / (double)g.N;
  loss_backward_kernel<<<dim3((unsigned)g.blocks), dim3(LTHREADS), 0, (hipStream_t)stream>>>(
      H, W, g.tiles_x, g.tiles_y, img, gt, maps, g.N, w_ssim != 0.0f, (float)((double)w_ssim * inv_n),
      (float)((double)w_l1 * inv_n), dL_dloss, dL_dimg);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

}  // extern "C"
