// gsr_bilagrid.hip -- per-image appearance compensation: the bilateral-grid slice (a 3 x 4 affine colour transform looked up
// by pixel position and luminance) with its backward, and the total-variation regulariser of the grids with its backward
// (DESIGN.md section 23): the gsr_bilagrid_* entry points of include/gsr.h, where the mathematics is stated.
//
// Decomposition.  The pixels of one image that fall into ONE (x, y) cell of the grid form a rectangle; `cell_of` below is
// the only place that decides which cell a pixel column / row belongs to, `cell_begin` inverts it.  A workgroup of 256
// threads owns the chunks s, s + S, s + 2 S, ... (256 pixels each, row-major inside the rectangle) of one cell of one image.
// Everything such a workgroup needs of the grid are the 4 x GZ x 12 floats at the cell's four corners: they are staged in
// LDS once ([z][corner][k]: the 24 floats a pixel needs per corner are contiguous) and no pixel gathers from global memory.
//
// Arithmetic.  Coordinates, weights, the interpolation and every sum are binary64; inputs and outputs are binary32.  The
// kernels are bound by their memory and LDS traffic, not by the arithmetic, and what they return is one rounding away from
// the exact value of the formula: the error of a float32 evaluation (the torch operators') is the yardstick of the tests.
//
// Backward, dL/dgrids.  No atomics.  Per chunk every thread stages its pixel's weights, colour and dL/dout in LDS; then
// wave w walks the 64 pixels it staged itself, in order, and lane (corner, k) < 48 adds the pixel's two contributions
// (z0 and z0 + 1) to ITS column of the wave's own LDS table [GZ][48] -- one owner per address, a fixed order.  At the end the
// workgroup adds its four tables in wave order and writes the [GZ][48] partial to its slot of the workspace;
// bila_reduce_kernel then adds, for every element of dL/dgrids, the partials of the (up to four) cells around its vertex over
// the images that selected the grid, in (image, cell, chunk-owner) order, and writes every element (zero where nothing was
// selected).  The same bits on every run.
//
// TV.  One thread per grid element: its forward differences (forward), or the four-to-six neighbours' (backward); block sums
// by a fixed tree into the workspace, a one-block finish in ascending order.
#include "../gsr_common.h"

using namespace gsr;

namespace {

constexpr int BG_THREADS = 256;
constexpr int BG_WAVES = BG_THREADS / WAVE;
constexpr int BG_MAX_XY = 32, BG_MAX_Z = 16;
constexpr int BG_K = 12;                  // the 3 x 4 matrix, k = 4 c + m
constexpr int BG_COLS = 4 * BG_K;         // (corner, k) columns of one z level: 48 lanes of a wave own one each
constexpr int BG_BLOCK_PIXELS = 1024;     // pixels a workgroup is sized for (four chunks)
constexpr int BG_MAX_SPLIT = 256;         // at most this many workgroups share one cell
static_assert(BG_COLS <= WAVE && BG_WAVES == 4, "one wave covers the columns; the flush adds four tables");

// The cell of pixel column (row) p of n along an axis of G vertices: x0 = min(floor(u (G - 1)), G - 2), u = (p + 0.5) / n.
__host__ __device__ inline double bila_coord(int p, int n, int G) { return ((double)p + 0.5) / (double)n * (double)(G - 1); }
__host__ __device__ inline int cell_of(int p, int n, int G) {
  const int c = (int)floor(bila_coord(p, n, G));
  return c > G - 2 ? G - 2 : c;
}
// The first p in [0, n] with cell_of(p) >= c (n if there is none); cell c holds the pixels [cell_begin(c), cell_begin(c + 1)).
__host__ __device__ inline int cell_begin(int c, int n, int G) {
  if (c <= 0) return 0;
  if (c >= G - 1) return n;
  int p = (int)((double)c * (double)n / (double)(G - 1));
  p = p < 0 ? 0 : (p > n ? n : p);
  while (p > 0 && cell_of(p - 1, n, G) >= c) --p;
  while (p < n && cell_of(p, n, G) < c) ++p;
  return p;
}

struct BilaPlan {
  int cells_x, cells_y, split;  // split = S: workgroups per cell
  int64_t blocks;               // B * cells * S
  size_t cols;                  // GZ * 48 doubles per workgroup partial
};

bool bila_dims_ok(int N, int GX, int GY, int GZ) {
  return N >= 1 && GX >= 2 && GX <= BG_MAX_XY && GY >= 2 && GY <= BG_MAX_XY && GZ >= 2 && GZ <= BG_MAX_Z;
}

bool bila_plan(int B, int H, int W, int GX, int GY, int GZ, BilaPlan* p) {
  if (B < 1 || H < 1 || W < 1 || !bila_dims_ok(1, GX, GY, GZ)) return false;
  if ((int64_t)H * (int64_t)W > (int64_t)0x7fffffff - BG_THREADS * (BG_MAX_SPLIT + 1)) return false;
  int mw = 0, mh = 0;
  for (int c = 0; c < GX - 1; ++c) {
    const int w = cell_begin(c + 1, W, GX) - cell_begin(c, W, GX);
    mw = w > mw ? w : mw;
  }
  for (int c = 0; c < GY - 1; ++c) {
    const int h = cell_begin(c + 1, H, GY) - cell_begin(c, H, GY);
    mh = h > mh ? h : mh;
  }
  const int64_t most = (int64_t)mw * (int64_t)mh;
  int64_t split = (most + BG_BLOCK_PIXELS - 1) / BG_BLOCK_PIXELS;
  split = split < 1 ? 1 : (split > BG_MAX_SPLIT ? BG_MAX_SPLIT : split);
  p->cells_x = GX - 1;
  p->cells_y = GY - 1;
  p->split = (int)split;
  p->blocks = (int64_t)B * (int64_t)p->cells_x * (int64_t)p->cells_y * split;
  p->cols = (size_t)GZ * BG_COLS;
  return p->blocks <= 0x7fffffff;
}

// A device-side index out of range selects the nearest valid grid: nothing is read or written outside `grids`.
__device__ __forceinline__ int clamp_index(const int64_t* __restrict__ idx, int b, int N) {
  const int64_t i = idx[b];
  return i < 0 ? 0 : (i > (int64_t)(N - 1) ? N - 1 : (int)i);
}

struct CellBlock {
  int b, cx, cy, s;          // image, cell, owner number within the cell
  int i0, j0, cw, npx;       // the cell's pixel rectangle: first row, first column, width, pixel count
};
__device__ __forceinline__ CellBlock cell_block(int H, int W, int GX, int GY, int S) {
  const unsigned cells = (unsigned)(GX - 1) * (unsigned)(GY - 1);
  const unsigned blk = blockIdx.x, q = blk / (unsigned)S, cell = q % cells;
  CellBlock c;
  c.s = (int)(blk - q * (unsigned)S);
  c.b = (int)(q / cells);
  c.cy = (int)(cell / (unsigned)(GX - 1));
  c.cx = (int)(cell - (unsigned)c.cy * (unsigned)(GX - 1));
  c.i0 = cell_begin(c.cy, H, GY);
  c.j0 = cell_begin(c.cx, W, GX);
  c.cw = cell_begin(c.cx + 1, W, GX) - c.j0;
  c.npx = c.cw * (cell_begin(c.cy + 1, H, GY) - c.i0);
  return c;
}

// the cell's four corners, every z and k -> sg[z][corner = 2 vy + vx][k]
__device__ __forceinline__ void stage_cell(float* sg, const float* __restrict__ grids, int n, const CellBlock& c, int GX, int GY,
                                           int GZ) {
  for (int i = (int)threadIdx.x; i < GZ * BG_COLS; i += BG_THREADS) {
    const int z = i / BG_COLS, r = i - z * BG_COLS, v = r / BG_K, k = r - v * BG_K;
    sg[i] = grids[((((size_t)n * BG_K + (size_t)k) * (size_t)GZ + (size_t)z) * (size_t)GY + (size_t)(c.cy + (v >> 1))) * (size_t)GX +
                  (size_t)(c.cx + (v & 1))];
  }
}

struct Pixel {
  double fx, fy, fz;
  float r, g, b;
  int z0;
  bool inside;  // 0 < gray < 1: the luminance clamp is not active
  size_t at;    // offset of the pixel in its plane
};
// pixel p of the cell's rectangle, image planes at img + 3 b H W
__device__ __forceinline__ Pixel load_pixel(const CellBlock& c, int p, int H, int W, int GX, int GY, int GZ,
                                            const float* __restrict__ img) {
  Pixel px;
  const int dy = p / c.cw, i = c.i0 + dy, j = c.j0 + (p - dy * c.cw);
  px.at = (size_t)i * (size_t)W + (size_t)j;
  const size_t plane = (size_t)H * (size_t)W;
  const float* q = img + (size_t)c.b * 3 * plane + px.at;
  px.r = q[0];
  px.g = q[plane];
  px.b = q[2 * plane];
  px.fx = bila_coord(j, W, GX) - (double)c.cx;
  px.fy = bila_coord(i, H, GY) - (double)c.cy;
  const double gray = 0.299 * (double)px.r + 0.587 * (double)px.g + 0.114 * (double)px.b;
  px.inside = gray > 0.0 && gray < 1.0;
  const double gz = fmin(fmax(gray, 0.0), 1.0) * (double)(GZ - 1);  // (NaN -> 0)
  int z0 = (int)floor(gz);
  z0 = z0 > GZ - 2 ? GZ - 2 : z0;
  px.z0 = z0;
  px.fz = gz - (double)z0;
  return px;
}

// lo[k], hi[k]: the bilinear (x, y) interpolation of the z levels z0 and z0 + 1
__device__ __forceinline__ void interp_xy(const float* sg, const Pixel& px, double (&lo)[BG_K], double (&hi)[BG_K]) {
  const double wx[2] = {1.0 - px.fx, px.fx}, wy[2] = {1.0 - px.fy, px.fy};
#pragma unroll
  for (int k = 0; k < BG_K; ++k) lo[k] = hi[k] = 0.0;
  const float4* base = reinterpret_cast<const float4*>(sg + px.z0 * BG_COLS);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const double w = wy[v >> 1] * wx[v & 1];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const float4 a = base[v * 3 + h], b = base[BG_COLS / 4 + v * 3 + h];
      lo[4 * h + 0] += w * (double)a.x;
      lo[4 * h + 1] += w * (double)a.y;
      lo[4 * h + 2] += w * (double)a.z;
      lo[4 * h + 3] += w * (double)a.w;
      hi[4 * h + 0] += w * (double)b.x;
      hi[4 * h + 1] += w * (double)b.y;
      hi[4 * h + 2] += w * (double)b.z;
      hi[4 * h + 3] += w * (double)b.w;
    }
  }
}

__global__ void __launch_bounds__(BG_THREADS)
bila_slice_forward_kernel(int H, int W, int N, int GX, int GY, int GZ, int S, const float* __restrict__ grids,
                          const int64_t* __restrict__ idx, const float* __restrict__ img, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sg[BG_MAX_Z * BG_COLS];
  const CellBlock c = cell_block(H, W, GX, GY, S);
  if (c.s * BG_THREADS >= c.npx) return;  // (uniform: nothing of this cell is this workgroup's)
  stage_cell(sg, grids, clamp_index(idx, c.b, N), c, GX, GY, GZ);
  __syncthreads();
  const size_t plane = (size_t)H * (size_t)W;
  for (int p = c.s * BG_THREADS + (int)threadIdx.x; p < c.npx; p += S * BG_THREADS) {
    const Pixel px = load_pixel(c, p, H, W, GX, GY, GZ, img);
    double lo[BG_K], hi[BG_K];
    interp_xy(sg, px, lo, hi);
    float* o = out + (size_t)c.b * 3 * plane + px.at;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      double a[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = lo[4 * ch + m] + px.fz * (hi[4 * ch + m] - lo[4 * ch + m]);
      o[ch * plane] = (float)(a[0] * (double)px.r + a[1] * (double)px.g + a[2] * (double)px.b + a[3]);
    }
  }
}

// dL_dimg (if not NULL) per pixel; the workgroup's [GZ][48] partial of dL_dgrids (if partial is not NULL) to its slot.
__global__ void __launch_bounds__(BG_THREADS)
bila_slice_backward_kernel(int H, int W, int N, int GX, int GY, int GZ, int S, const float* __restrict__ grids,
                           const int64_t* __restrict__ idx, const float* __restrict__ img, const float* __restrict__ dout,
                           float* __restrict__ dimg, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float sg[BG_MAX_Z * BG_COLS];
  __shared__ double tab[BG_WAVES][BG_MAX_Z * BG_COLS];
  __shared__ double s_w[4][BG_THREADS], s_fz[BG_THREADS];  // the pixel's four (x, y) corner weights, its z fraction
  __shared__ float s_go[3][BG_THREADS], s_col[4][BG_THREADS];
  __shared__ int s_z0[BG_THREADS];
  const CellBlock c = cell_block(H, W, GX, GY, S);
  const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int cols = GZ * BG_COLS;
  if (partial != nullptr)
    for (int i = tid; i < BG_WAVES * BG_MAX_Z * BG_COLS; i += BG_THREADS) (&tab[0][0])[i] = 0.0;
  if (dimg != nullptr && c.s * BG_THREADS < c.npx) stage_cell(sg, grids, clamp_index(idx, c.b, N), c, GX, GY, GZ);
  __syncthreads();
  const size_t plane = (size_t)H * (size_t)W;
  // lane (corner v, k = 4 ch + m) of every wave owns column `lane` of the wave's table
  const int v = lane / BG_K, k = lane - v * BG_K, ch = k >> 2, m = k & 3;
  for (int p0 = c.s * BG_THREADS; p0 < c.npx; p0 += S * BG_THREADS) {  // (uniform)
    const int p = p0 + tid;
    int z0 = -1;
    if (p < c.npx) {
      const Pixel px = load_pixel(c, p, H, W, GX, GY, GZ, img);
      const float* gq = dout + (size_t)c.b * 3 * plane + px.at;
      const float g0 = gq[0], g1 = gq[plane], g2 = gq[2 * plane];
      if (dimg != nullptr) {
        double lo[BG_K], hi[BG_K];
        interp_xy(sg, px, lo, hi);
        const double go[3] = {(double)g0, (double)g1, (double)g2};
        const double col[3] = {(double)px.r, (double)px.g, (double)px.b};
        double direct[3] = {0.0, 0.0, 0.0}, guide = 0.0;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          double dz = hi[4 * cc + 3] - lo[4 * cc + 3];  // d out_cc / d gz
#pragma unroll
          for (int mm = 0; mm < 3; ++mm) {
            const double d = hi[4 * cc + mm] - lo[4 * cc + mm];
            direct[mm] += go[cc] * (lo[4 * cc + mm] + px.fz * d);
            dz += d * col[mm];
          }
          guide += go[cc] * dz;
        }
        guide = px.inside ? guide * (double)(GZ - 1) : 0.0;
        float* o = dimg + (size_t)c.b * 3 * plane + px.at;
        o[0] = (float)(direct[0] + 0.299 * guide);
        o[plane] = (float)(direct[1] + 0.587 * guide);
        o[2 * plane] = (float)(direct[2] + 0.114 * guide);
      }
      z0 = px.z0;
      s_w[0][tid] = (1.0 - px.fy) * (1.0 - px.fx);
      s_w[1][tid] = (1.0 - px.fy) * px.fx;
      s_w[2][tid] = px.fy * (1.0 - px.fx);
      s_w[3][tid] = px.fy * px.fx;
      s_fz[tid] = px.fz;
      s_go[0][tid] = g0;
      s_go[1][tid] = g1;
      s_go[2][tid] = g2;
      s_col[0][tid] = px.r;
      s_col[1][tid] = px.g;
      s_col[2][tid] = px.b;
      s_col[3][tid] = 1.0f;
    }
    s_z0[tid] = z0;
    __syncthreads();
    if (partial != nullptr && lane < BG_COLS) {
      double* mine = &tab[wave][lane];
      const int first = wave * WAVE, left = c.npx - p0 - first;  // (the pixels of a chunk are valid up to its end)
      const int valid = left > WAVE ? WAVE : left;
#pragma unroll 4
      for (int q = first; q < first + valid; ++q) {
        const int z = s_z0[q];
        const double fz = s_fz[q];
        const double val = s_w[v][q] * ((double)s_go[ch][q] * (double)s_col[m][q]);
        mine[z * BG_COLS] += val * (1.0 - fz);
        mine[(z + 1) * BG_COLS] += val * fz;
      }
    }
    __syncthreads();
  }
  if (partial != nullptr) {
    double* dst = partial + (size_t)blockIdx.x * (size_t)cols;
    for (int i = tid; i < cols; i += BG_THREADS) dst[i] = ((tab[0][i] + tab[1][i]) + tab[2][i]) + tab[3][i];
  }
}

// One thread per element of dL_dgrids, k fastest (as the partials lie): the sum over the images b (ascending) that selected
// grid n, the cells around the vertex (cy, then cx, ascending) and the cell's workgroups (ascending).
__global__ void __launch_bounds__(BG_THREADS)
bila_reduce_kernel(int B, int N, int GX, int GY, int GZ, int S, const int64_t* __restrict__ idx,
                   const double* __restrict__ partial, float* __restrict__ dgrids) {
  const size_t per_grid = (size_t)BG_K * GZ * GY * GX, total = (size_t)N * per_grid;
  const size_t e = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
  if (e >= total) return;
  const int n = (int)(e / per_grid);
  unsigned r = (unsigned)(e - (size_t)n * per_grid);
  const int k = (int)(r % BG_K);
  r /= BG_K;
  const int z = (int)(r % (unsigned)GZ);
  r /= (unsigned)GZ;
  const int x = (int)(r % (unsigned)GX), y = (int)(r / (unsigned)GX);
  const size_t cells = (size_t)(GX - 1) * (size_t)(GY - 1), cols = (size_t)GZ * BG_COLS;
  double sum = 0.0;
  for (int b = 0; b < B; ++b) {
    if (clamp_index(idx, b, N) != n) continue;
    for (int vy = 1; vy >= 0; --vy) {
      const int cy = y - vy;
      if (cy < 0 || cy > GY - 2) continue;
      for (int vx = 1; vx >= 0; --vx) {
        const int cx = x - vx;
        if (cx < 0 || cx > GX - 2) continue;
        const double* src = partial + (((size_t)b * cells + (size_t)cy * (size_t)(GX - 1) + (size_t)cx) * (size_t)S) * cols +
                            (size_t)z * BG_COLS + (size_t)((vy * 2 + vx) * BG_K + k);
        for (int s = 0; s < S; ++s) sum += src[(size_t)s * cols];
      }
    }
  }
  dgrids[((((size_t)n * BG_K + (size_t)k) * (size_t)GZ + (size_t)z) * (size_t)GY + (size_t)y) * (size_t)GX + (size_t)x] = (float)sum;
}

// ---- total variation ----
struct TvDims {
  int GX, GY, GZ;
  double sz, sy, sx;  // 1 / count_d: differenced elements of ONE grid along z, y, x
};
TvDims tv_dims(int GX, int GY, int GZ) {
  TvDims d;
  d.GX = GX;
  d.GY = GY;
  d.GZ = GZ;
  d.sz = 1.0 / ((double)BG_K * (GZ - 1) * GY * GX);
  d.sy = 1.0 / ((double)BG_K * GZ * (GY - 1) * GX);
  d.sx = 1.0 / ((double)BG_K * GZ * GY * (GX - 1));
  return d;
}

// block sums of sum_d (forward difference along d)^2 / count_d, one element per thread, a fixed tree
__global__ void __launch_bounds__(BG_THREADS)
bila_tv_forward_kernel(size_t total, TvDims d, const float* __restrict__ grids, double* __restrict__ partial) {
  __shared__ double red[BG_THREADS];
  const size_t e = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
  double t = 0.0;
  if (e < total) {
    const int x = (int)(e % (unsigned)d.GX), y = (int)((e / (unsigned)d.GX) % (unsigned)d.GY);
    const int z = (int)((e / ((unsigned)d.GX * (unsigned)d.GY)) % (unsigned)d.GZ);
    const double a = (double)grids[e];
    if (z + 1 < d.GZ) {
      const double f = (double)grids[e + (size_t)d.GY * d.GX] - a;
      t += f * f * d.sz;
    }
    if (y + 1 < d.GY) {
      const double f = (double)grids[e + (size_t)d.GX] - a;
      t += f * f * d.sy;
    }
    if (x + 1 < d.GX) {
      const double f = (double)grids[e + 1] - a;
      t += f * f * d.sx;
    }
  }
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = BG_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// out1 = (sum of the block sums, thread t the slots t, t + 256, ... ascending, then a fixed tree) / N
__global__ void __launch_bounds__(BG_THREADS)
bila_tv_finish_kernel(const double* __restrict__ partial, int n, double inv_grids, float* __restrict__ out1) {
  __shared__ double red[BG_THREADS];
  double t = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += BG_THREADS) t += partial[i];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = BG_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out1[0] = (float)(red[0] * inv_grids);
}

// dL_dgrids[e] = g / N * sum_d 2 / count_d * ((e - next_d) + (e - previous_d)), g = *dL_dtv read on the device; the bracket
// does not depend on g.
__global__ void __launch_bounds__(BG_THREADS)
bila_tv_backward_kernel(size_t total, TvDims d, double inv_grids, const float* __restrict__ grids,
                        const float* __restrict__ dL_dtv, float* __restrict__ dgrids) {
  const size_t e = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
  if (e >= total) return;
  const int x = (int)(e % (unsigned)d.GX), y = (int)((e / (unsigned)d.GX) % (unsigned)d.GY);
  const int z = (int)((e / ((unsigned)d.GX * (unsigned)d.GY)) % (unsigned)d.GZ);
  const size_t sy = (size_t)d.GX, sz = (size_t)d.GY * d.GX;
  const double a = (double)grids[e];
  double t = 0.0, u = 0.0;
  if (z + 1 < d.GZ) u += a - (double)grids[e + sz];
  if (z > 0) u += a - (double)grids[e - sz];
  t += u * d.sz;
  u = 0.0;
  if (y + 1 < d.GY) u += a - (double)grids[e + sy];
  if (y > 0) u += a - (double)grids[e - sy];
  t += u * d.sy;
  u = 0.0;
  if (x + 1 < d.GX) u += a - (double)grids[e + 1];
  if (x > 0) u += a - (double)grids[e - 1];
  t += u * d.sx;
  dgrids[e] = (float)((double)dL_dtv[0] * (2.0 * inv_grids * t));
}

bool tv_blocks(int N, int GX, int GY, int GZ, size_t* total, int64_t* blocks) {
  if (!bila_dims_ok(N, GX, GY, GZ)) return false;
  *total = (size_t)N * BG_K * GZ * GY * GX;
  *blocks = (int64_t)((*total + BG_THREADS - 1) / BG_THREADS);
  return *blocks <= 0x7fffffff;
}

}  // namespace

extern "C" {

int gsr_bilagrid_workspace_size(int B, int H, int W, int GX, int GY, int GZ, size_t* bytes) {
  BilaPlan p;
  if (bytes == nullptr || !bila_plan(B, H, W, GX, GY, GZ, &p)) return GSR_ERR_BAD_ARGUMENT;
  *bytes = (size_t)p.blocks * p.cols * sizeof(double);
  return GSR_OK;
}

int gsr_bilagrid_slice_forward(void* stream, int B, int H, int W, int N, int GX, int GY, int GZ, const float* grids,
                               const int64_t* idx, const float* img, float* out) {
  BilaPlan p;
  if (!bila_plan(B, H, W, GX, GY, GZ, &p) || N < 1 || grids == nullptr || idx == nullptr || img == nullptr || out == nullptr)
    return GSR_ERR_BAD_ARGUMENT;
  bila_slice_forward_kernel<<<dim3((unsigned)p.blocks), dim3(BG_THREADS), 0, (hipStream_t)stream>>>(H, W, N, GX, GY, GZ, p.split,
                                                                                                    grids, idx, img, out);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_bilagrid_slice_backward(void* stream, int B, int H, int W, int N, int GX, int GY, int GZ, const float* grids,
                                const int64_t* idx, const float* img, const float* dL_dout, void* workspace, float* dL_dimg,
                                float* dL_dgrids) {
  BilaPlan p;
  if (!bila_plan(B, H, W, GX, GY, GZ, &p) || N < 1 || grids == nullptr || idx == nullptr || img == nullptr || dL_dout == nullptr)
    return GSR_ERR_BAD_ARGUMENT;
  if (dL_dgrids != nullptr && (workspace == nullptr || ((uintptr_t)workspace & 7u) != 0)) return GSR_ERR_BAD_ARGUMENT;
  if (dL_dimg == nullptr && dL_dgrids == nullptr) return GSR_OK;
  hipStream_t s = (hipStream_t)stream;
  double* partial = dL_dgrids != nullptr ? (double*)workspace : nullptr;
  bila_slice_backward_kernel<<<dim3((unsigned)p.blocks), dim3(BG_THREADS), 0, s>>>(H, W, N, GX, GY, GZ, p.split, grids, idx, img,
                                                                                   dL_dout, dL_dimg, partial);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  if (dL_dgrids == nullptr) return GSR_OK;
  const size_t total = (size_t)N * BG_K * GZ * GY * GX;
  const size_t blocks = (total + BG_THREADS - 1) / BG_THREADS;
  if (blocks > 0x7fffffffu) return GSR_ERR_BAD_ARGUMENT;
  bila_reduce_kernel<<<dim3((unsigned)blocks), dim3(BG_THREADS), 0, s>>>(B, N, GX, GY, GZ, p.split, idx, partial, dL_dgrids);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_bilagrid_tv_workspace_size(int N, int GX, int GY, int GZ, size_t* bytes) {
  size_t total;
  int64_t blocks;
  if (bytes == nullptr || !tv_blocks(N, GX, GY, GZ, &total, &blocks)) return GSR_ERR_BAD_ARGUMENT;
  *bytes = (size_t)blocks * sizeof(double);
  return GSR_OK;
}

int gsr_bilagrid_tv_forward(void* stream, int N, int GX, int GY, int GZ, const float* grids, void* workspace, float* out1) {
  size_t total;
  int64_t blocks;
  if (!tv_blocks(N, GX, GY, GZ, &total, &blocks) || grids == nullptr || workspace == nullptr || out1 == nullptr ||
      ((uintptr_t)workspace & 7u) != 0)
    return GSR_ERR_BAD_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  bila_tv_forward_kernel<<<dim3((unsigned)blocks), dim3(BG_THREADS), 0, s>>>(total, tv_dims(GX, GY, GZ), grids, (double*)workspace);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  bila_tv_finish_kernel<<<dim3(1), dim3(BG_THREADS), 0, s>>>((const double*)workspace, (int)blocks, 1.0 / (double)N, out1);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_bilagrid_tv_backward(void* stream, int N, int GX, int GY, int GZ, const float* grids, const float* dL_dtv,
                             float* dL_dgrids) {
  size_t total;
  int64_t blocks;
  if (!tv_blocks(N, GX, GY, GZ, &total, &blocks) || grids == nullptr || dL_dtv == nullptr || dL_dgrids == nullptr)
    return GSR_ERR_BAD_ARGUMENT;
  bila_tv_backward_kernel<<<dim3((unsigned)blocks), dim3(BG_THREADS), 0, (hipStream_t)stream>>>(
      total, tv_dims(GX, GY, GZ), 1.0 / (double)N, grids, dL_dtv, dL_dgrids);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

}  // extern "C"
