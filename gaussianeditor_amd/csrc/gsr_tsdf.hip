// gsr_tsdf.hip -- TSDF fusion of rendered depth into a dense volume, and the mesh of its zero level by marching
// tetrahedra; the gsr_tsdf_* entry points of include/gsr.h, where the mathematics is stated.
//
// Integrate.  One launch over all V views.  A block of TS_BX x TS_BY x TS_BZ lanes owns that brick of lattice points, z
// fastest (TS_BZ consecutive floats: one 128-byte line per (x, y) row of the brick): a lane keeps its point's tsdf, weight
// and colour in registers across all views and stores them once -- the volume moves once, not V times.  The camera records
// (the GSR_FILTER3D_CAMERA_DOUBLES layout) are staged TS_CHUNK at a time in LDS and read at a wave-uniform address.  The
// depth, alpha and colour of the nearest pixel are gathered; a brick projects to a small patch of the image, so the
// gathers stay in the caches.  Projection and comparisons binary64, the running average binary32 (-ffp-contract=off: one
// IEEE operation per operator, in the order include/gsr.h states).  No atomics.
// Mesh.  count / scan / apply as gsr_compact.hip does it, over the lattice points in blocks of MT_ROWS:
//   mark      one lane per cube: the six Kuhn tetrahedra; the faces of the cube (a byte) and, per crossed edge of an emitting
//             tetrahedron, the edge's bit in the 7-bit mask of its lower lattice point (an integer atomic OR on the word
//             that holds four masks: marks do not depend on the order);
//   count     per block the number of marked edges and of faces;  scan: one block, the exclusive prefixes and the totals;
//   vertices  per lattice point the id of its first vertex (block prefix + scan in the block), kept for the faces, and the
//             vertices themselves;  faces: per cube the tetrahedra again, vertex id = first id of the lower point + the
//             rank of the edge's bit in that point's mask.
// The orientation of every (tetrahedron, case) is a compile-time table computed in integers from the edge midpoints.
#include <math.h>

#include "gsr_common.h"

using namespace gsr;

namespace {

constexpr int TS_BX = 2, TS_BY = 4, TS_BZ = 32;      // the brick of a block (gaussianeditor_amd/tsdf.py: BLOCK_DIMS)
constexpr int TS_THREADS = TS_BX * TS_BY * TS_BZ;
constexpr int TS_CHUNK = 32;                         // cameras per LDS stage (tsdf.py: CAMERAS_PER_CHUNK)
constexpr int TS_CAM = GSR_FILTER3D_CAMERA_DOUBLES;  // doubles per camera record
constexpr int MT_ROWS = 1024;                        // lattice points per block of the mesh kernels (tsdf.py: MESH_ROWS_PER_BLOCK)

static_assert(TS_THREADS == 256 && TS_CAM == 20, "the brick is four waves; the record layout is that of include/gsr.h");

struct TsdfGrid {
  int nx, ny, nz;
  float ox, oy, oz, vs;
};

// ------------------------------------------------------------------------------------------------------------------------
// integrate
// ------------------------------------------------------------------------------------------------------------------------
template <bool ALPHA, bool COLOR>
__global__ void __launch_bounds__(TS_THREADS)
tsdf_integrate_kernel(const TsdfGrid g, int gy, int gz, int V, int H, int W, const float* __restrict__ depth,
                      const float* __restrict__ alpha, const float* __restrict__ color, const double* __restrict__ cameras,
                      double trunc, double alpha_min, float max_weight, float* __restrict__ tsdf, float* __restrict__ weight,
                      float* __restrict__ vol_color) {
  __shared__ double cam[TS_CHUNK * TS_CAM];
  const unsigned b = blockIdx.x;
  const int bz = (int)(b % (unsigned)gz), by = (int)((b / (unsigned)gz) % (unsigned)gy), bx = (int)(b / ((unsigned)gz * (unsigned)gy));
  const int t = (int)threadIdx.x;
  const int i = bx * TS_BX + (t >> 7), j = by * TS_BY + ((t >> 5) & 3), k = bz * TS_BZ + (t & 31);
  const bool live = i < g.nx && j < g.ny && k < g.nz;
  const size_t N = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
  const size_t n = live ? ((size_t)i * (size_t)g.ny + (size_t)j) * (size_t)g.nz + (size_t)k : 0;
  const double x = (double)g.ox + (double)g.vs * (double)i;
  const double y = (double)g.oy + (double)g.vs * (double)j;
  const double z = (double)g.oz + (double)g.vs * (double)k;
  float f = 1.0f, w = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  if (live) {
    f = tsdf[n];
    w = weight[n];
    if (COLOR) {
      c0 = vol_color[n];
      c1 = vol_color[N + n];
      c2 = vol_color[2 * N + n];
    }
  }
  const double near_plane = (double)0.2f;
  const double cx = ((double)W - 1.0) * 0.5, cy = ((double)H - 1.0) * 0.5;
  const size_t HW = (size_t)H * (size_t)W;
  bool touched = false;
  for (int v0 = 0; v0 < V; v0 += TS_CHUNK) {
    const int nc = V - v0 < TS_CHUNK ? V - v0 : TS_CHUNK;
    __syncthreads();  // (the chunk before this one has been read by every wave)
    for (int e = t; e < nc * TS_CAM; e += TS_THREADS) cam[e] = cameras[(size_t)v0 * TS_CAM + (size_t)e];
    __syncthreads();
    if (!live) continue;
    for (int c = 0; c < nc; ++c) {
      const double* m = cam + c * TS_CAM;  // [0..11] M[r][k] at 3 r + k; [12] fx; [13] fy
      const double zc = ((x * m[2] + y * m[5]) + z * m[8]) + m[11];
      if (!(zc > near_plane)) continue;
      const double p0 = ((x * m[0] + y * m[3]) + z * m[6]) + m[9];
      const double p1 = ((x * m[1] + y * m[4]) + z * m[7]) + m[10];
      const double fu = floor(((p0 / zc) * m[12] + cx) + 0.5);
      const double fv = floor(((p1 / zc) * m[13] + cy) + 0.5);
      if (!(fu >= 0.0 && fu < (double)W && fv >= 0.0 && fv < (double)H)) continue;  // (a NaN fails every comparison)
      const size_t pix = (size_t)(int)fv * (size_t)W + (size_t)(int)fu;
      const size_t view = (size_t)(v0 + c);
      float d = depth[view * HW + pix];
      if (ALPHA) {
        const float a = alpha[view * HW + pix];
        if ((double)a < alpha_min) continue;
        d = d / a;
      }
      if (!(d > 0.0f)) continue;
      const double sdf = (double)d - zc;
      if (sdf < -trunc) continue;
      const double r = sdf / trunc;
      const float obs = (float)(r < 1.0 ? r : 1.0);
      float w1 = w + 1.0f;
      f = (f * w + obs) / w1;
      if (COLOR) {
        const float* px = color + view * 3 * HW + pix;
        c0 = (c0 * w + px[0]) / w1;
        c1 = (c1 * w + px[HW]) / w1;
        c2 = (c2 * w + px[2 * HW]) / w1;
      }
      if (max_weight > 0.0f) w1 = w1 < max_weight ? w1 : max_weight;
      w = w1;
      touched = true;
    }
  }
  if (live && touched) {
    tsdf[n] = f;
    weight[n] = w;
    if (COLOR) {
      vol_color[n] = c0;
      vol_color[N + n] = c1;
      vol_color[2 * N + n] = c2;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// marching tetrahedra: the tables
// ------------------------------------------------------------------------------------------------------------------------
// A cube's corner is the code dx | dy << 1 | dz << 2.  Tetrahedron t (axis permutation pi, lexicographic) is the path
// 0, e_pi1, e_pi1 + e_pi2, 7.
struct MtTables {
  uint8_t corner[6][4];  // corner codes of the path
  uint16_t flip[6];      // bit `case`: the triangle (A,B,C) is emitted as (A,C,B)
  uint8_t ntri[16];      // triangles of a case
  uint8_t tri[16][6];    // their edges before any flip, three per triangle: p | q << 2 for the path positions p < q
};

constexpr MtTables mt_build() {
  MtTables T{};
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int m = 0; m < 16; ++m) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int p = 0; p < 4; ++p) {
      if ((m >> p) & 1) in[ni++] = p;
      else out[no++] = p;
    }
    int e[6][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
    T.ntri[m] = (uint8_t)((ni == 0 || ni == 4) ? 0 : (ni == 2 ? 2 : 1));
    if (ni == 1) {
      for (int q = 0; q < 3; ++q) { e[q][0] = in[0]; e[q][1] = out[q]; }
    } else if (ni == 3) {
      for (int q = 0; q < 3; ++q) { e[q][0] = out[0]; e[q][1] = in[q]; }
    } else if (ni == 2) {
      // a = in[0] < b = in[1], c = out[0] < d = out[1]: q0 = (a,c), q1 = (a,d), q2 = (b,d), q3 = (b,c); (q0,q1,q2), (q0,q2,q3)
      const int quad[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
      const int order[6] = {0, 1, 2, 0, 2, 3};
      for (int q = 0; q < 6; ++q) { e[q][0] = quad[order[q]][0]; e[q][1] = quad[order[q]][1]; }
    }
    for (int q = 0; q < 6; ++q) {
      const int lo = e[q][0] < e[q][1] ? e[q][0] : e[q][1], hi = e[q][0] < e[q][1] ? e[q][1] : e[q][0];
      T.tri[m][q] = (uint8_t)(lo | (hi << 2));
    }
  }
  for (int t = 0; t < 6; ++t) {
    T.corner[t][0] = 0;
    T.corner[t][1] = (uint8_t)(1 << perm[t][0]);
    T.corner[t][2] = (uint8_t)((1 << perm[t][0]) | (1 << perm[t][1]));
    T.corner[t][3] = 7;
    T.flip[t] = 0;
    for (int m = 1; m < 15; ++m) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
      for (int p = 0; p < 4; ++p) {
        if ((m >> p) & 1) in[ni++] = p;
        else out[no++] = p;
      }
      // the first triangle's three edges
      int e[3][2] = {{0, 0}, {0, 0}, {0, 0}};
      for (int q = 0; q < 3; ++q) { e[q][0] = T.tri[m][q] & 3; e[q][1] = T.tri[m][q] >> 2; }
      // doubled midpoints A, B, C; n = (B - A) x (C - A); dir = ni sum(outside) - no sum(inside) (a positive multiple of
      // mean(outside) - mean(inside))
      int P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int q = 0; q < 3; ++q)
        for (int a = 0; a < 3; ++a)
          P[q][a] = ((T.corner[t][e[q][0]] >> a) & 1) + ((T.corner[t][e[q][1]] >> a) & 1);
      const int ux = P[1][0] - P[0][0], uy = P[1][1] - P[0][1], uz = P[1][2] - P[0][2];
      const int vx = P[2][0] - P[0][0], vy = P[2][1] - P[0][1], vz = P[2][2] - P[0][2];
      const int nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
      int dir[3] = {0, 0, 0};
      for (int a = 0; a < 3; ++a) {
        int so = 0, si = 0;
        for (int q = 0; q < no; ++q) so += (T.corner[t][out[q]] >> a) & 1;
        for (int q = 0; q < ni; ++q) si += (T.corner[t][in[q]] >> a) & 1;
        dir[a] = ni * so - no * si;
      }
      const int dot = nx * dir[0] + ny * dir[1] + nz * dir[2];
      if (dot < 0) T.flip[t] = (uint16_t)(T.flip[t] | (1u << m));
    }
  }
  return T;
}

__constant__ const MtTables MT = mt_build();
// kind of the edge direction d = (upper corner code) ^ (lower corner code): 100, 010, 001, 110, 101, 011, 111 as dx dy dz
__constant__ const int8_t MT_KIND[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// the direction of a kind, as a corner code
__constant__ const uint8_t MT_DIR[7] = {1, 2, 4, 3, 5, 6, 7};

struct MeshWork {
  uint64_t* totals;     // (2) vertices, faces
  uint32_t* mask;       // (ceil(N / 4)) four 7-bit edge masks per word
  uint8_t* fcount;      // (N) faces of the cube whose corner the point is
  uint32_t* vbase;      // (N) id of the point's first vertex
  uint32_t* block_cnt;  // (2 nb) marked edges, then faces, per block
  uint32_t* block_off;  // (2 nb) their exclusive prefixes
  size_t bytes;
};
__host__ __device__ inline MeshWork carve_mesh(void* base, int64_t N) {
  char* p = (char*)base;
  const size_t nb = ((size_t)N + MT_ROWS - 1) / MT_ROWS;
  MeshWork w;
  size_t off = 0;
  w.totals = (uint64_t*)(p + off);     off += 256;
  w.mask = (uint32_t*)(p + off);       off += align_up(sizeof(uint32_t) * (((size_t)N + 3) / 4));
  w.fcount = (uint8_t*)(p + off);      off += align_up((size_t)N);
  w.vbase = (uint32_t*)(p + off);      off += align_up(sizeof(uint32_t) * (size_t)N);
  w.block_cnt = (uint32_t*)(p + off);  off += align_up(sizeof(uint32_t) * 2 * nb);
  w.block_off = (uint32_t*)(p + off);  off += align_up(sizeof(uint32_t) * 2 * nb);
  w.bytes = off;
  return w;
}

struct Cube {
  int i, j, k;
  bool is_cube;
  uint32_t inside, observed;  // bit = corner code
};

__device__ __forceinline__ int64_t corner_offset(const TsdfGrid& g, int code) {
  return (int64_t)(code & 1) * g.ny * g.nz + (int64_t)((code >> 1) & 1) * g.nz + (int64_t)(code >> 2);
}

__device__ __forceinline__ Cube load_cube(const TsdfGrid& g, int64_t n, int64_t N, const float* __restrict__ tsdf,
                                          const float* __restrict__ weight) {
  Cube c;
  c.inside = c.observed = 0;
  c.is_cube = false;
  c.i = c.j = c.k = 0;
  if (n >= N) return c;
  c.k = (int)(n % g.nz);
  c.j = (int)((n / g.nz) % g.ny);
  c.i = (int)(n / ((int64_t)g.nz * g.ny));
  c.is_cube = c.i < g.nx - 1 && c.j < g.ny - 1 && c.k < g.nz - 1;
  if (!c.is_cube) return c;
#pragma unroll
  for (int code = 0; code < 8; ++code) {
    const int64_t m = n + corner_offset(g, code);
    c.inside |= (tsdf[m] < 0.0f ? 1u : 0u) << code;
    c.observed |= (weight[m] > 0.0f ? 1u : 0u) << code;
  }
  return c;
}

// case of tetrahedron t (bit p: path point p inside), 0 where it emits nothing
__device__ __forceinline__ uint32_t tet_case(const Cube& c, int t) {
  uint32_t m = 0, obs = 1;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int code = MT.corner[t][p];
    m |= ((c.inside >> code) & 1u) << p;
    obs &= (c.observed >> code) & 1u;
  }
  return (obs && m != 15u) ? m : 0u;
}

__global__ void __launch_bounds__(MT_ROWS)
mesh_mark_kernel(const TsdfGrid g, int64_t N, const float* __restrict__ tsdf, const float* __restrict__ weight,
                 uint32_t* __restrict__ mask, uint8_t* __restrict__ fcount) {
  const int64_t n = (int64_t)blockIdx.x * MT_ROWS + threadIdx.x;
  if (n >= N) return;
  const Cube c = load_cube(g, n, N, tsdf, weight);
  uint32_t faces = 0;
  uint64_t marks = 0;  // byte = corner code: the kinds of the crossed edges that start there
  if (c.is_cube && c.inside != 0u && c.inside != 255u) {
    for (int t = 0; t < 6; ++t) {
      const uint32_t m = tet_case(c, t);
      if (m == 0u) continue;
      faces += __popc(m) == 2 ? 2u : 1u;
      for (int p = 0; p < 3; ++p)
        for (int q = p + 1; q < 4; ++q)
          if (((m >> p) ^ (m >> q)) & 1u) {
            const int lo = MT.corner[t][p], kind = MT_KIND[MT.corner[t][q] ^ lo];
            marks |= 1ull << (lo * 8 + kind);
          }
    }
  }
  fcount[n] = (uint8_t)faces;
  if (marks == 0ull) return;
#pragma unroll
  for (int code = 0; code < 8; ++code) {
    const uint32_t bits = (uint32_t)(marks >> (code * 8)) & 0x7fu;
    if (bits != 0u) {
      const int64_t m = n + corner_offset(g, code);
      atomicOr(mask + (m >> 2), bits << ((int)(m & 3) * 8));
    }
  }
}

__device__ __forceinline__ uint32_t point_mask(const uint32_t* __restrict__ mask, int64_t n) {
  return (mask[n >> 2] >> ((int)(n & 3) * 8)) & 0x7fu;
}

// per block: marked edges | faces << 16 (at most 7 and 12 per point, 1024 points: both sums fit 16 bits)
__global__ void __launch_bounds__(MT_ROWS)
mesh_count_kernel(int64_t N, const uint32_t* __restrict__ mask, const uint8_t* __restrict__ fcount, int64_t nb,
                  uint32_t* __restrict__ block_cnt) {
  __shared__ uint32_t smem[MT_ROWS / 64 + 1];
  const int64_t n = (int64_t)blockIdx.x * MT_ROWS + threadIdx.x;
  const uint32_t v = n < N ? (uint32_t)__popc(point_mask(mask, n)) | ((uint32_t)fcount[n] << 16) : 0u;
  uint32_t total;
  (void)block_excl_scan_u32<MT_ROWS>(v, &total, smem);
  if (threadIdx.x == 0) {
    block_cnt[blockIdx.x] = total & 0xffffu;
    block_cnt[nb + blockIdx.x] = total >> 16;
  }
}

// one block: the exclusive prefixes of both count arrays and their totals (at most 7 N and 12 N < 2^32 for 7 N < 2^31)
__global__ void __launch_bounds__(1024)
mesh_scan_kernel(int64_t nb, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off, uint64_t* __restrict__ totals) {
  __shared__ uint32_t smem[1024 / 64 + 1];
  for (int which = 0; which < 2; ++which) {
    uint64_t carry = 0;
    for (int64_t base = 0; base < nb; base += 1024) {
      const int64_t i = base + threadIdx.x;
      const uint32_t v = i < nb ? cnt[which * nb + i] : 0u;
      uint32_t chunk;
      const uint32_t ex = block_excl_scan_u32<1024>(v, &chunk, smem);
      if (i < nb) off[which * nb + i] = (uint32_t)carry + ex;
      carry += chunk;
    }
    if (threadIdx.x == 0) totals[which] = carry;
  }
}

__global__ void __launch_bounds__(MT_ROWS)
mesh_vertices_kernel(const TsdfGrid g, int64_t N, const float* __restrict__ tsdf, const float* __restrict__ vol_color,
                     const uint32_t* __restrict__ mask, const uint32_t* __restrict__ block_off, uint32_t* __restrict__ vbase,
                     int64_t n_vertices, float* __restrict__ vertices, float* __restrict__ colors) {
  __shared__ uint32_t smem[MT_ROWS / 64 + 1];
  const int64_t n = (int64_t)blockIdx.x * MT_ROWS + threadIdx.x;
  const uint32_t bits = n < N ? point_mask(mask, n) : 0u;
  uint32_t total;
  const uint32_t first = block_off[blockIdx.x] + block_excl_scan_u32<MT_ROWS>((uint32_t)__popc(bits), &total, smem);
  if (n >= N) return;
  vbase[n] = first;
  if (bits == 0u) return;
  const int k = (int)(n % g.nz), j = (int)((n / g.nz) % g.ny), i = (int)(n / ((int64_t)g.nz * g.ny));
  const float lower[3] = {(float)i, (float)j, (float)k}, origin[3] = {g.ox, g.oy, g.oz};
  const float f0 = tsdf[n];
  uint32_t id = first;
  for (int kind = 0; kind < 7; ++kind) {
    if (!((bits >> kind) & 1u)) continue;
    const int d = MT_DIR[kind];
    const int64_t m = n + corner_offset(g, d);  // (a marked edge belongs to a cube: m < N unless the workspace is not this grid's)
    if (m >= N) break;
    const float f1 = tsdf[m];
    const float t = f0 / (f0 - f1);
    if ((int64_t)id < n_vertices) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float step = ((d >> a) & 1) ? t : 0.0f;
        vertices[(size_t)id * 3 + a] = origin[a] + g.vs * (lower[a] + step);
      }
      if (colors != nullptr) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float ca = vol_color[(size_t)a * (size_t)N + (size_t)n], cb = vol_color[(size_t)a * (size_t)N + (size_t)m];
          colors[(size_t)id * 3 + a] = ca + t * (cb - ca);
        }
      }
    }
    ++id;
  }
}

// id of the vertex on the edge between path points p < q of tetrahedron t of the cube at n
__device__ __forceinline__ int32_t edge_vertex(const TsdfGrid& g, int64_t n, int t, int p, int q, const uint32_t* __restrict__ mask,
                                               const uint32_t* __restrict__ vbase) {
  const int lo = MT.corner[t][p], kind = MT_KIND[MT.corner[t][q] ^ lo];
  const int64_t m = n + corner_offset(g, lo);
  return (int32_t)(vbase[m] + (uint32_t)__popc(point_mask(mask, m) & ((1u << kind) - 1u)));
}

__global__ void __launch_bounds__(MT_ROWS)
mesh_faces_kernel(const TsdfGrid g, int64_t N, const float* __restrict__ tsdf, const float* __restrict__ weight,
                  const uint32_t* __restrict__ mask, const uint8_t* __restrict__ fcount, const uint32_t* __restrict__ vbase,
                  const uint32_t* __restrict__ block_off, int64_t n_faces, int32_t* __restrict__ faces) {
  __shared__ uint32_t smem[MT_ROWS / 64 + 1];
  const int64_t n = (int64_t)blockIdx.x * MT_ROWS + threadIdx.x;
  const uint32_t mine = n < N ? (uint32_t)fcount[n] : 0u;
  uint32_t total;
  uint32_t id = block_off[blockIdx.x] + block_excl_scan_u32<MT_ROWS>(mine, &total, smem);
  if (mine == 0u) return;
  const Cube c = load_cube(g, n, N, tsdf, weight);
  const uint32_t end = id + mine;
  for (int t = 0; t < 6; ++t) {
    const uint32_t m = tet_case(c, t);
    if (m == 0u) continue;
    const bool flip = (MT.flip[t] >> m) & 1u;
    const int nt = MT.ntri[m];
    for (int f = 0; f < nt; ++f) {
      int32_t v[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int code = MT.tri[m][3 * f + e];
        v[e] = edge_vertex(g, n, t, code & 3, code >> 2, mask, vbase);
      }
      if (id < end && (int64_t)id < n_faces) {
        faces[(size_t)id * 3 + 0] = v[0];
        faces[(size_t)id * 3 + 1] = flip ? v[2] : v[1];
        faces[(size_t)id * 3 + 2] = flip ? v[1] : v[2];
      }
      ++id;
    }
  }
}

bool ts_aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// the number of lattice points, -1 where an extent is below 1 or the product exceeds 2^31 - 1
int64_t ts_points(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1) return -1;
  const int64_t a = (int64_t)nx * (int64_t)ny;
  if (a > 0x7fffffffll) return -1;
  const int64_t N = a * (int64_t)nz;
  return N > 0x7fffffffll ? -1 : N;
}

bool ts_grid(TsdfGrid& g, int nx, int ny, int nz, float ox, float oy, float oz, float vs) {
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.ox = ox; g.oy = oy; g.oz = oz; g.vs = vs;
  return isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(vs);
}

}  // namespace

extern "C" {

int gsr_tsdf_integrate(void* stream, int nx, int ny, int nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                       int V, int H, int W, const float* depth, const float* alpha, const float* color, const double* cameras,
                       double trunc, double alpha_min, float max_weight, float* tsdf, float* weight, float* vol_color) {
  TsdfGrid g;
  const int64_t N = ts_points(nx, ny, nz);
  if (N < 0 || !ts_grid(g, nx, ny, nz, origin_x, origin_y, origin_z, voxel_size) || !(voxel_size > 0.0f)) return GSR_ERR_BAD_ARGUMENT;
  if (V < 1 || H < 1 || W < 1 || (int64_t)V * (int64_t)H * (int64_t)W > 0x7fffffffll) return GSR_ERR_BAD_ARGUMENT;
  if (!(trunc > 0.0) || !isfinite(trunc) || !(alpha_min > 0.0) || !isfinite(alpha_min) || !(max_weight >= 0.0f) || !isfinite(max_weight))
    return GSR_ERR_BAD_ARGUMENT;
  if (depth == nullptr || cameras == nullptr || tsdf == nullptr || weight == nullptr || (color == nullptr) != (vol_color == nullptr))
    return GSR_ERR_BAD_ARGUMENT;
  if (!ts_aligned4(depth) || !ts_aligned4(alpha) || !ts_aligned4(color) || !ts_aligned4(tsdf) || !ts_aligned4(weight) ||
      !ts_aligned4(vol_color) || ((uintptr_t)cameras & 7u) != 0)
    return GSR_ERR_BAD_ARGUMENT;
  const int64_t gx = (nx + TS_BX - 1) / TS_BX, gy = (ny + TS_BY - 1) / TS_BY, gz = (nz + TS_BZ - 1) / TS_BZ;
  const int64_t blocks = gx * gy * gz;  // (at most 2^31 - 1 points, so far below 2^63)
  if (blocks > 0x7fffffffll) return GSR_ERR_BAD_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(TS_THREADS);
#define TS_LAUNCH(A, C)                                                                                                    \
  tsdf_integrate_kernel<A, C><<<grid, block, 0, s>>>(g, (int)gy, (int)gz, V, H, W, depth, alpha, color, cameras, trunc, alpha_min, \
                                                     max_weight, tsdf, weight, vol_color)
  if (alpha != nullptr && color != nullptr) TS_LAUNCH(true, true);
  else if (alpha != nullptr) TS_LAUNCH(true, false);
  else if (color != nullptr) TS_LAUNCH(false, true);
  else TS_LAUNCH(false, false);
#undef TS_LAUNCH
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

int gsr_tsdf_mesh_workspace_size(int nx, int ny, int nz, size_t* bytes) {
  const int64_t N = ts_points(nx, ny, nz);
  if (bytes == nullptr || N < 0) return GSR_ERR_BAD_ARGUMENT;
  if (7 * N >= (1ll << 31)) return GSR_ERR_TOO_MANY;
  *bytes = carve_mesh(nullptr, N).bytes;
  return GSR_OK;
}

int gsr_tsdf_mesh_count(void* stream, int nx, int ny, int nz, const float* tsdf, const float* weight, void* workspace,
                        int64_t* counts_host) {
  if (counts_host == nullptr) return GSR_ERR_BAD_ARGUMENT;
  counts_host[0] = counts_host[1] = 0;
  TsdfGrid g;
  const int64_t N = ts_points(nx, ny, nz);
  if (N < 0) return GSR_ERR_BAD_ARGUMENT;
  if (7 * N >= (1ll << 31)) return GSR_ERR_TOO_MANY;
  if (tsdf == nullptr || weight == nullptr || workspace == nullptr || !ts_aligned4(tsdf) || !ts_aligned4(weight) ||
      ((uintptr_t)workspace & 255u) != 0)
    return GSR_ERR_BAD_ARGUMENT;
  (void)ts_grid(g, nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f);
  const MeshWork w = carve_mesh(workspace, N);
  const int64_t nb = (N + MT_ROWS - 1) / MT_ROWS;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(w.mask, 0, sizeof(uint32_t) * (((size_t)N + 3) / 4), s) != hipSuccess) return GSR_ERR_HIP;
  mesh_mark_kernel<<<dim3((unsigned)nb), dim3(MT_ROWS), 0, s>>>(g, N, tsdf, weight, w.mask, w.fcount);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  mesh_count_kernel<<<dim3((unsigned)nb), dim3(MT_ROWS), 0, s>>>(N, w.mask, w.fcount, nb, w.block_cnt);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  mesh_scan_kernel<<<dim3(1), dim3(1024), 0, s>>>(nb, w.block_cnt, w.block_off, w.totals);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  uint64_t totals[2] = {0, 0};
  if (hipMemcpyAsync(totals, w.totals, sizeof(totals), hipMemcpyDeviceToHost, s) != hipSuccess) return GSR_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return GSR_ERR_HIP;
  if (totals[1] > 0x7fffffffull) return GSR_ERR_TOO_MANY;
  counts_host[0] = (int64_t)totals[0];
  counts_host[1] = (int64_t)totals[1];
  return GSR_OK;
}

int gsr_tsdf_mesh_emit(void* stream, int nx, int ny, int nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                       const float* tsdf, const float* weight, const float* vol_color, const void* workspace,
                       int64_t n_vertices, int64_t n_faces, float* vertices, float* colors, int32_t* faces) {
  TsdfGrid g;
  const int64_t N = ts_points(nx, ny, nz);
  if (N < 0 || !ts_grid(g, nx, ny, nz, origin_x, origin_y, origin_z, voxel_size)) return GSR_ERR_BAD_ARGUMENT;
  if (7 * N >= (1ll << 31)) return GSR_ERR_TOO_MANY;
  if (n_vertices < 0 || n_faces < 0 || n_vertices > 7 * N || n_faces > 0x7fffffffll) return GSR_ERR_BAD_ARGUMENT;
  if (n_vertices == 0 && n_faces == 0) return GSR_OK;
  if (tsdf == nullptr || weight == nullptr || workspace == nullptr || vertices == nullptr || faces == nullptr ||
      (colors != nullptr && vol_color == nullptr))
    return GSR_ERR_BAD_ARGUMENT;
  if (!ts_aligned4(tsdf) || !ts_aligned4(weight) || !ts_aligned4(vol_color) || !ts_aligned4(vertices) || !ts_aligned4(colors) ||
      !ts_aligned4(faces) || ((uintptr_t)workspace & 255u) != 0)
    return GSR_ERR_BAD_ARGUMENT;
  const MeshWork w = carve_mesh(const_cast<void*>(workspace), N);
  const int64_t nb = (N + MT_ROWS - 1) / MT_ROWS;
  hipStream_t s = (hipStream_t)stream;
  mesh_vertices_kernel<<<dim3((unsigned)nb), dim3(MT_ROWS), 0, s>>>(g, N, tsdf, vol_color, w.mask, w.block_off, w.vbase, n_vertices,
                                                                    vertices, colors);
  if (hipGetLastError() != hipSuccess) return GSR_ERR_HIP;
  mesh_faces_kernel<<<dim3((unsigned)nb), dim3(MT_ROWS), 0, s>>>(g, N, tsdf, weight, w.mask, w.fcount, w.vbase, w.block_off + nb,
                                                                 n_faces, faces);
  return hipGetLastError() != hipSuccess ? GSR_ERR_HIP : GSR_OK;
}

}  // extern "C"
