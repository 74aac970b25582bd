// gsr_blend.hip -- the per-tile alpha-compositing kernels: K6 (forward), K7 (backward),
// K12 (semantic tracing / apply_weights).
//
// CDNA4 mapping.  The reference runs one 256-thread block per 16x16 tile (8 warps of 32)
// with block-wide barriers around a shared-memory staging buffer.  Here the unit of work is
// ONE WAVE64 = one 8x8 pixel quadrant of a tile, launched as a single-wave workgroup:
//   * the forward and the tracing kernel have no workgroup barrier (a one-wave workgroup's
//     s_barrier is free), each quadrant terminates as soon as ITS 64 pixels are opaque,
//     and the CU's wave slots are refilled at wave granularity;
//   * 8x8 is the most compact 64-pixel footprint, so the exec mask stays coherent and the
//     "no lane contributes" early-outs (scalar branches on a 64-bit ballot) fire often;
//   * each wave stages 64 sorted instances at a time in LDS (3 x float4 per instance, read
//     back as uniform-address ds_read_b128 broadcasts);
//   * the kernels are PERSISTENT: a fixed number of single-wave workgroups (a few per SIMD)
//     pull (tile, quadrant) items from eight per-XCD queues (one relaxed agent-scope atomic
//     per item).  Tiles are queued longest-list-first (gsr_binning.hip: tile_worklist_kernel)
//     and dealt round-robin to the XCD queues, so every XCD gets the same amount of work, the
//     heavy quadrants start first and the light ones fill the gaps (the instance lists are
//     heavy-tailed: with one workgroup per quadrant most SIMDs idle through a long tail);
//     the four quadrants of a tile are consecutive items of ONE queue, so they gather the same
//     Gaussians through the same 4 MiB L2.  Which wave runs an item never affects results;
//   * the backward runs one 4-wave workgroup per tile: the quadrant waves reduce the 9 per-Gaussian gradient terms of
//     four entries at a time across their 64 lanes (wave_sum4_pack: the 36 values are packed pairwise, by selects and DPP
//     adds inside the rows and three lane swaps across them, until every lane holds one total), add their totals with one
//     ds_add_f32 into a per-chunk LDS accumulator (double-buffered by chunk parity: one workgroup barrier per chunk),
//     and ONE global atomic per (tile, instance, term) leaves the CU -- the reference issues one per pixel.
#include <limits.h>

#include <atomic>
#include <type_traits>

#include "gsr_kernels.h"

namespace gsr {

struct PixelWave {
  int tile, px, py;
  bool inside;
};

// (tile, quadrant) -> this lane's pixel.  Returns false if the quadrant lies outside the image.
__device__ __forceinline__ bool setup_wave(const BlendArgs& a, uint32_t tile, uint32_t quad, PixelWave& pw) {
  const int tx = (int)(tile % (uint32_t)a.gx), ty = (int)(tile / (uint32_t)a.gx);
  const int lane = lane_id();
  pw.tile = (int)tile;
  pw.px = tx * TILE + (int)(quad & 1u) * QUAD + (lane & 7);
  pw.py = ty * TILE + (int)(quad >> 1) * QUAD + (lane >> 3);
  pw.inside = pw.px < a.W && pw.py < a.H;
  return __any(pw.inside) != 0;
}

// The pixels of one forward / trace item and its pixel rectangle (the cull test of the blend loops starts from the pixels
// that are live, live_pixel_box, which lie inside it).  `code` = quad | sub << 2 from
// run_work_queue.  The item covers its quadrant, or -- when the image is small (SPLIT, image-wide) -- rows [4 s, 4 s + 4) /
// the 4x4 block s of it: lanes outside the part are switched off (pw.inside), the box shrinks with it.  Returns false if
// no pixel is inside the image.
struct ItemBox {
  float qx0, qy0, qw, qh;
};
template <int SPLIT>
__device__ __forceinline__ bool setup_item(const BlendArgs& a, uint32_t tile, uint32_t code, PixelWave& pw, ItemBox& b) {
  constexpr uint32_t split = (uint32_t)SPLIT;
  const uint32_t sub = (code >> 2) & 3u;
  if (!setup_wave(a, tile, code & 3u, pw)) return false;
  const int lane = lane_id();
  b.qx0 = (float)(pw.px - (lane & 7));
  b.qy0 = (float)(pw.py - (lane >> 3));
  b.qw = b.qh = (float)(QUAD - 1);
  if (split == 2u) {  // rows [4 sub, 4 sub + 4)
    pw.inside = pw.inside && ((uint32_t)(lane >> 5) == sub);
    b.qy0 += 4.0f * (float)sub;
    b.qh = 3.0f;
  } else if (split == 4u) {  // the 4x4 block (sub & 1, sub >> 1)
    pw.inside = pw.inside && ((uint32_t)((lane >> 2) & 1) == (sub & 1u)) && ((uint32_t)(lane >> 5) == (sub >> 1));
    b.qx0 += 4.0f * (float)(sub & 1u);
    b.qy0 += 4.0f * (float)(sub >> 1);
    b.qw = b.qh = 3.0f;
  }
  return true;
}

// Persistent work loop.  Queue x (one per XCD) owns entries x, x+8, x+16, ... of work_order;
// its cursor counts quadrant items (4 per non-empty tile) and then, if `with_empty`, one item
// per empty tile.  A wave serves the queue of the XCD it happens to run on (HW_REG_XCC_ID, a
// placement hint only: any wave may run any item).
// Called by ONE thread of every workgroup after its last (failed) pop: the workgroup that retires last puts the
// cursors of this queue kind back to zero, so the next launch of the kind finds them cleared without a memset.
// (Every pop of every other workgroup has returned before that workgroup's retire increment is issued.)
// Two levels, one counter per 64 workgroups and one on top: memory-side atomics on ONE line serialise at ~6 ns
// each, which for 4096 workgroups retiring together measured 20 us on the tail of the forward kernel.
__device__ __forceinline__ void retire_queue(uint32_t* queue) {
  const uint32_t nwg = gridDim.x, grp = blockIdx.x >> 6, ngrp = (nwg + 63u) >> 6;
  if (ngrp > (uint32_t)QUEUE_GROUPS) return;  // (launchers fall back to a memset for such grids)
  const uint32_t gsize = min(64u, nwg - (grp << 6));
  uint32_t* top = queue + 8 * QUEUE_STRIDE;
  uint32_t* gcnt = queue + 9 * QUEUE_STRIDE;
  if (__hip_atomic_fetch_add(gcnt + grp * QUEUE_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gsize - 1u) return;
  if (__hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ngrp - 1u) return;
#pragma unroll
  for (int x = 0; x < 8; ++x) __hip_atomic_store(queue + x * QUEUE_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint32_t i = 0; i < ngrp; ++i)
    __hip_atomic_store(gcnt + i * QUEUE_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Work distribution.  The persistent workgroups are placed deterministically (measured with the per-wave profile,
// tools/wave_profile.py): with `units` = number of SIMDs (single-wave workgroups) or CUs (4-wave workgroups), block b
// runs on unit b % units in residency slot b / units, and on XCD b % 8.  A kernel ends when its busiest SIMD does, and
// with a plain longest-first queue every wave's FIRST item is one of the few very long lists (the per-item work is
// extremely skewed: mean 80 evaluated entries per quadrant, maximum 800), so the four long items that happen to share
// a SIMD decide the run time: the busiest SIMD carried 1.83x the mean load.
// Hence the first item of every workgroup is assigned, not popped: slot 0 of unit u takes item u of its XCD's queue,
// slot 1 item 2n-1-u, slot 2 item 2n+u, slot 3 item 4n-1-u, ... (n = units per XCD): every unit gets one item from
// each stratum of the sorted list, folded so that the sums even out.  Everything after the first W n items is popped
// dynamically.  The assignment is a permutation of [0, W n) whatever the real placement is, so results never depend on it.
__device__ __forceinline__ uint32_t first_item_of_block(uint32_t units, uint32_t& queue_x, uint32_t& first_dynamic) {
  if (units == 0u) {  // no assignment: everything is popped
    queue_x = 0u;
    first_dynamic = 0u;
    return 0xffffffffu;
  }
  const uint32_t n = units / 8u, W = gridDim.x / units;  // launchers guarantee units % 8 == 0, gridDim.x % units == 0
  const uint32_t b = blockIdx.x, slot = b / units, u = (b % units) / 8u;
  queue_x = b % 8u;
  first_dynamic = W * n;
  return (slot & 1u) ? (slot + 1u) * n - 1u - u : slot * n + u;
}

// HW_REG_XCC_ID[3:0]: the XCD the wave runs on (the queue it serves: & 7; the profile records keep all four bits)
__device__ __forceinline__ uint32_t xcc_id() { return (uint32_t)__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20); }
// A kernel argument's float once per kernel, in a scalar register: `bg` of K6 / K7.  (Read at its uses, hipcc cannot prove
// that the image stores do not alias it: it re-loaded each component between two stores and waited for everything in flight
// each time.)
__device__ __forceinline__ float wave_uniform(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
// The pixels of a whole tile, quadrant by quadrant: f(pixel index, H W) for every lane whose pixel lies inside the image (the
// empty-tile items of the forward kernels: background only / zeros).
template <class F>
__device__ __forceinline__ void for_each_pixel_of_tile(const BlendArgs& a, uint32_t tile, F&& f) {
  for (uint32_t q = 0; q < 4; ++q) {
    PixelWave pw;
    if (!setup_wave(a, tile, q, pw)) continue;
    if (pw.inside) f((size_t)pw.py * a.W + pw.px, (size_t)a.H * a.W);
  }
}

template <int SPLIT, class F>
__device__ __forceinline__ void run_work_queue(const BlendArgs& a, bool with_empty, F&& item) {
  const uint32_t nwork = a.work_meta[0];
  const uint32_t T = (uint32_t)(a.gx * a.gy);
  const uint32_t nempty = with_empty ? T - nwork : 0u;
  // queue x (one per XCD) owns entries x, x+8, ... of work_order: 4 quadrant items per non-empty tile, then one item
  // per empty tile
  // Granularity: a quadrant is one item, unless that leaves fewer than two items per persistent wave (small images,
  // e.g. the editor's 512x512 views: 1024 tiles for 4096 waves): then every quadrant is cut into 2 (8x4 pixels) or 4
  // (4x4) items, which trades lane utilisation the chip is not using anyway for shorter serial chains and finer
  // culling.  The item code passed on is quad | sub << 2, decoded by the item function.
  constexpr uint32_t split = (uint32_t)SPLIT;  // chosen by the launcher from the number of tiles of the image
  constexpr uint32_t per_tile = 4u * split;
  auto run_item = [&](uint32_t x, uint32_t q) __attribute__((always_inline)) -> bool {
    const uint32_t n_x = nwork > x ? (nwork - x + 7u) / 8u : 0u;
    const uint32_t e_x = nempty > x ? (nempty - x + 7u) / 8u : 0u;
    if (q >= per_tile * n_x + e_x) return false;
    if (q < per_tile * n_x) {
      const uint32_t t = q / per_tile, r = q - t * per_tile;  // r = quad * split + sub
      item(a.work_order[x + 8u * t], split == 1u ? r : ((r / split) | ((r % split) << 2)), false);
    } else {
      item(a.work_order[nwork + x + 8u * (q - per_tile * n_x)], 0u, true);
    }
    return true;
  };
  uint32_t x0, base;
  const uint32_t q0 = first_item_of_block((uint32_t)a.units, x0, base);
  (void)run_item(x0, q0);
  // then serve the queue of the XCD the wave really runs on (HW_REG_XCC_ID; equal to x0 on this chip)
  const uint32_t x = xcc_id() & 7u;
  uint32_t* head = a.queue + x * QUEUE_STRIDE;
  for (;;) {
    uint32_t q = 0;
    if (lane_id() == 0) q = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    q = (uint32_t)__builtin_amdgcn_readfirstlane((int)q);
    if (!run_item(x, base + q)) break;
  }
  if (a.self_reset && lane_id() == 0) retire_queue(a.queue);
}

// Read-only tables of an earlier kernel, read through the SCALAR cache at a wave-uniform index (s_load: its counter,
// lgkmcnt, is independent of the vector memory counter, so picking such a value up never waits for stores or gathers).
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t scalar_load(const uint32_t* p, uint32_t i) {
  return ((__attribute__((address_space(4))) const uint32_t*)(uintptr_t)p)[i];
}
__device__ __forceinline__ uint2 scalar_load(const uint2* p, uint32_t i) {
  const u32x2 v = ((__attribute__((address_space(4))) const u32x2*)(uintptr_t)p)[i];
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint4 scalar_load(const uint4* p, uint32_t i) {
  const u32x4 v = ((__attribute__((address_space(4))) const u32x4*)(uintptr_t)p)[i];
  return make_uint4(v.x, v.y, v.z, v.w);
}

// max over the 64 lanes of a wave, in every lane: 6 v_max_u32_dpp (row_shr 1, 2, 4, 8, row_bcast 15 / 31) + one v_readlane
__device__ __forceinline__ uint32_t wave_max_u32_dpp(uint32_t v) {
  auto step = [](uint32_t w, auto ctrl, auto rows) __attribute__((always_inline)) {
    return max(w, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, decltype(ctrl)::value, decltype(rows)::value, 0xf, false));
  };
  v = step(v, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
  v = step(v, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
  v = step(v, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
  v = step(v, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
  v = step(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
  v = step(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

constexpr int GROUP = 4;  // survivors processed per inner-loop iteration
// Sums each of four per-lane values over the 64 lanes of the wave, 10 instructions for all four
// instead of 4 x 6: two v_permlane32_swap + adds fold the half-waves (a,c | b,d), one
// v_permlane16_swap + add folds row pairs so that row r of the wave holds 16 partial sums of
// value r (wave_fold4_to_rows), then 4 row_shr DPP adds finish each row.  The total of value r ends up in lane 16 r + 15.
__device__ __forceinline__ float wave_fold4_to_rows(float a, float b, float c, float d) {
  unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
  unsigned uc = __builtin_bit_cast(unsigned, c), ud = __builtin_bit_cast(unsigned, d);
  {
    auto r = __builtin_amdgcn_permlane32_swap(ua, uc, false, false);  // ua = [a_lo|c_lo], uc = [a_hi|c_hi]
    ua = r[0];
    uc = r[1];
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(ub, ud, false, false);
    ub = r[0];
    ud = r[1];
  }
  const float x = __builtin_bit_cast(float, ua) + __builtin_bit_cast(float, uc);  // lanes 0-31: a, 32-63: c
  const float y = __builtin_bit_cast(float, ub) + __builtin_bit_cast(float, ud);  // lanes 0-31: b, 32-63: d
  unsigned ux = __builtin_bit_cast(unsigned, x), uy = __builtin_bit_cast(unsigned, y);
  {
    auto r = __builtin_amdgcn_permlane16_swap(ux, uy, false, false);  // ux rows [x0,y0,x2,y2], uy rows [x1,y1,x3,y3]
    ux = r[0];
    uy = r[1];
  }
  return __builtin_bit_cast(float, ux) + __builtin_bit_cast(float, uy);  // rows: a, b, c, d
}
__device__ __forceinline__ float wave_sum4_to_rows(float a, float b, float c, float d) {
  float z = wave_fold4_to_rows(a, b, c, d);
  z = dpp_add<0x111>(z);
  z = dpp_add<0x112>(z);
  z = dpp_add<0x114>(z);
  z = dpp_add<0x118>(z);
  return z;
}

// The same for NM values per entry at once (K7: the raw moments), PACKED: a reduction that finishes one total per register
// leaves 63 of its 64 lanes unused, and the v_permlane*_swap that the transposed form spends on every value are the
// expensive instructions of K7's group body (about 10 cycles of a SIMD each against 2 for a DPP add or a select,
// profiles/r07_a_packed_reduction.md).  Here the 4 NM registers are PAIRED at every distance: a lane keeps the first
// register of a pair if its bit of that distance is clear and the second if it is set, and one add takes the same register
// from the lane that differs in that bit (which kept the other one); a register without a partner adds its own other half.
// Six stages halve 4 NM registers to one:
//   inside a row, distances 8, 4, 2, 1: two selects and one DPP add per pair -- row_ror:8 (lane ^ 8), row_half_mirror
//   (7 - lane inside the 8-lane half: flips bit 2 and stays inside the half, which row_ror:4 does not), quad_perm [2,3,0,1]
//   (lane ^ 2), quad_perm [1,0,3,2] (lane ^ 1);
//   across the rows, 32 and 16: one v_permlane32_swap / v_permlane16_swap and one add per pair, no select (the swap itself
//   leaves the first register's two halves in the lower lanes and the second's in the upper ones).
// For NM = 9: 36 -> 18 -> 9 -> 5 -> 3 -> 2 -> 1 registers, 35 DPP adds, 66 selects and 3 swaps where one chain per value
// took 36 DPP adds and 27 swaps (MASKED, below: 62 DPP adds and 12 selects).  Afterwards lane i holds the complete wave total of ONE value, pack_lanes<NM>() says which.
template <int S> struct PackStage {
  static_assert(S == 8 || S == 4 || S == 2 || S == 1 || S == 32 || S == 16, "distances inside a wave");
  static constexpr int ctrl = S == 8 ? 0x128 : S == 4 ? 0x141 : S == 2 ? 0x4E : 0xB1;
  static constexpr int partner(int lane) { return S == 4 ? lane ^ 7 : lane ^ S; }
  static constexpr bool second(int lane) { return (lane & S) != 0; }
};
// MASKED (K7): at distances 8 and 4 the choice is made by the add's own destination write instead of by two selects.  Bits 3
// and 2 of the lane number are bank-granular (a DPP bank: four adjacent lanes of a row), so for a pair (a, b)
//     v_add_f32_dpp a, a, a row_ror:8 bank_mask:0x3        lanes with bit 3 clear: a + a of the partner
//     v_add_f32_dpp a, b, b row_ror:8 bank_mask:0xc        lanes with bit 3 set:   b + b of the partner
// leaves in `a` what the two selects and the add leave in the pair's result: the same adds on the same operands in the same
// lanes (distance 4: row_half_mirror, masks 0x5 / 0xa).  The destination is `a` in both: the second add reads `b` alone.
// hipcc does not form the masked add from __builtin_amdgcn_update_dpp (it keeps a masked v_mov_b32_dpp beside the adds),
// hence the asm; it cannot see into the string either, so every statement opens with the two wait states a DPP read of a
// VGPR needs after a VALU write of it (s_nop 1, what hipcc puts there itself), and takes up to ten pairs (the 30-operand
// limit of a statement) to pay them once per twenty adds.  A pair reads nothing that its own statement writes.
#define GSR_MP_ADD(i, CTRL, M0, M1)                                                             \
  "v_add_f32_dpp %[a" #i "], %[a" #i "], %[a" #i "] " CTRL " row_mask:0xf bank_mask:" M0 "\n\t" \
  "v_add_f32_dpp %[a" #i "], %[b" #i "], %[b" #i "] " CTRL " row_mask:0xf bank_mask:" M1 "\n\t"
#define GSR_MP_A(i) [a##i] "+v"(z[2 * (p0 + i)])
#define GSR_MP_B(i) [b##i] "v"(z[2 * (p0 + i) + 1])
#define GSR_MP_S1(C, M0, M1) GSR_MP_ADD(0, C, M0, M1)
#define GSR_MP_A1 GSR_MP_A(0)
#define GSR_MP_B1 GSR_MP_B(0)
#define GSR_MP_S2(C, M0, M1) GSR_MP_S1(C, M0, M1) GSR_MP_ADD(1, C, M0, M1)
#define GSR_MP_A2 GSR_MP_A1, GSR_MP_A(1)
#define GSR_MP_B2 GSR_MP_B1, GSR_MP_B(1)
#define GSR_MP_S3(C, M0, M1) GSR_MP_S2(C, M0, M1) GSR_MP_ADD(2, C, M0, M1)
#define GSR_MP_A3 GSR_MP_A2, GSR_MP_A(2)
#define GSR_MP_B3 GSR_MP_B2, GSR_MP_B(2)
#define GSR_MP_S4(C, M0, M1) GSR_MP_S3(C, M0, M1) GSR_MP_ADD(3, C, M0, M1)
#define GSR_MP_A4 GSR_MP_A3, GSR_MP_A(3)
#define GSR_MP_B4 GSR_MP_B3, GSR_MP_B(3)
#define GSR_MP_S5(C, M0, M1) GSR_MP_S4(C, M0, M1) GSR_MP_ADD(4, C, M0, M1)
#define GSR_MP_A5 GSR_MP_A4, GSR_MP_A(4)
#define GSR_MP_B5 GSR_MP_B4, GSR_MP_B(4)
#define GSR_MP_S6(C, M0, M1) GSR_MP_S5(C, M0, M1) GSR_MP_ADD(5, C, M0, M1)
#define GSR_MP_A6 GSR_MP_A5, GSR_MP_A(5)
#define GSR_MP_B6 GSR_MP_B5, GSR_MP_B(5)
#define GSR_MP_S7(C, M0, M1) GSR_MP_S6(C, M0, M1) GSR_MP_ADD(6, C, M0, M1)
#define GSR_MP_A7 GSR_MP_A6, GSR_MP_A(6)
#define GSR_MP_B7 GSR_MP_B6, GSR_MP_B(6)
#define GSR_MP_S8(C, M0, M1) GSR_MP_S7(C, M0, M1) GSR_MP_ADD(7, C, M0, M1)
#define GSR_MP_A8 GSR_MP_A7, GSR_MP_A(7)
#define GSR_MP_B8 GSR_MP_B7, GSR_MP_B(7)
#define GSR_MP_S9(C, M0, M1) GSR_MP_S8(C, M0, M1) GSR_MP_ADD(8, C, M0, M1)
#define GSR_MP_A9 GSR_MP_A8, GSR_MP_A(8)
#define GSR_MP_B9 GSR_MP_B8, GSR_MP_B(8)
#define GSR_MP_S10(C, M0, M1) GSR_MP_S9(C, M0, M1) GSR_MP_ADD(9, C, M0, M1)
#define GSR_MP_A10 GSR_MP_A9, GSR_MP_A(9)
#define GSR_MP_B10 GSR_MP_B9, GSR_MP_B(9)
#define GSR_MP_CASE(K)                                                                                                   \
  if constexpr (COUNT == K) {                                                                                            \
    if constexpr (S == 8) asm("s_nop 1\n\t" GSR_MP_S##K("row_ror:8", "0x3", "0xc") : GSR_MP_A##K : GSR_MP_B##K);          \
    else asm("s_nop 1\n\t" GSR_MP_S##K("row_half_mirror", "0x5", "0xa") : GSR_MP_A##K : GSR_MP_B##K);                     \
  }
// pairs p0 .. p0 + COUNT - 1 of z: z[2 p] <- the pair's result
template <int S, int COUNT>
__device__ __forceinline__ void masked_pairs(float* z, int p0) {
  static_assert((S == 8 || S == 4) && COUNT >= 1 && COUNT <= 10, "a row stage whose bit is bank-granular; one statement");
  GSR_MP_CASE(1) GSR_MP_CASE(2) GSR_MP_CASE(3) GSR_MP_CASE(4) GSR_MP_CASE(5)
  GSR_MP_CASE(6) GSR_MP_CASE(7) GSR_MP_CASE(8) GSR_MP_CASE(9) GSR_MP_CASE(10)
}
template <int S, int PAIRS, int P0 = 0>
__device__ __forceinline__ void masked_stage(float* z) {
  if constexpr (PAIRS > 0) {
    constexpr int count = PAIRS < 10 ? PAIRS : 10;
    masked_pairs<S, count>(z, P0);
    masked_stage<S, PAIRS - count, P0 + count>(z);
  }
}
template <int S, int N, bool MASKED = false>
__device__ __forceinline__ void pack_stage(float* z, int lane) {
  if constexpr (MASKED && (S == 8 || S == 4)) {
    masked_stage<S, N / 2>(z);
#pragma unroll
    for (int p = 1; p < N / 2; ++p) z[p] = z[2 * p];
    if (N & 1) z[N / 2] = dpp_add<PackStage<S>::ctrl>(z[N - 1]);
  } else if constexpr (S >= 16) {
    auto fold = [](float a, float b) __attribute__((always_inline)) {
      const unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
      // (the two results go through scalars: __builtin_bit_cast applied to r[1] itself reads r[0] with this compiler)
      if constexpr (S == 32) {
        auto r = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);  // [a_lo | b_lo], [a_hi | b_hi]
        const unsigned r0 = r[0], r1 = r[1];
        return __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
      } else {
        auto r = __builtin_amdgcn_permlane16_swap(ua, ub, false, false);  // rows [a0, b0, a2, b2], [a1, b1, a3, b3]
        const unsigned r0 = r[0], r1 = r[1];
        return __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
      }
    };
#pragma unroll
    for (int p = 0; p < N / 2; ++p) z[p] = fold(z[2 * p], z[2 * p + 1]);
    if (N & 1) z[N / 2] = fold(z[N - 1], z[N - 1]);
  } else {
    auto other = [](float x) __attribute__((always_inline)) {  // folds into the add: v_add_f32_dpp
      return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), PackStage<S>::ctrl, 0xf, 0xf, true));
    };
    const bool second = (lane & S) != 0;
#pragma unroll
    for (int p = 0; p < N / 2; ++p) {
      const float a = z[2 * p], b = z[2 * p + 1];
      const float keep = second ? b : a, give = second ? a : b;
      z[p] = keep + other(give);
    }
    if (N & 1) z[N / 2] = z[N - 1] + other(z[N - 1]);
  }
}
template <int NM, bool MASKED = false>
__device__ __forceinline__ float wave_sum4_pack(const float (&v)[NM][GROUP]) {
  static_assert(GROUP == 4 && NM >= 1 && NM <= 16, "4 NM values, at most one per lane");
  const int lane = lane_id();
  constexpr int N0 = NM * GROUP, N1 = (N0 + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2, N5 = (N4 + 1) / 2;
  static_assert((N5 + 1) / 2 == 1, "six halvings leave one register");
  float z[N0];  // value k of entry u: register GROUP k + u -- the first two stages fold the four entries of a value
#pragma unroll
  for (int k = 0; k < NM; ++k)
#pragma unroll
    for (int u = 0; u < GROUP; ++u) z[GROUP * k + u] = v[k][u];
  pack_stage<8, N0, MASKED>(z, lane);
  pack_stage<4, N1, MASKED>(z, lane);
  pack_stage<2, N2>(z, lane);
  pack_stage<1, N3>(z, lane);
  pack_stage<32, N4>(z, lane);
  pack_stage<16, N5>(z, lane);
  return z[0];
}
// Which value a lane ends up with: the same pairing, run on indices.  ok = false if a stage would add two different values
// (the lane an add reads from must have kept the same register) -- the static_asserts below rule that out.
//   adds: the lanes that add their total to the accumulators -- of the lanes that hold the same value, the lowest;
//   term_bit / entry_bit: bit planes over the lanes of the value's index k and of its entry u.
struct PackLanes {
  uint64_t adds, term_bit[4], entry_bit[2];
  int value[WAVE];
  bool ok;
};
template <int NM>
constexpr PackLanes pack_lanes() {
  constexpr int N0 = NM * GROUP;
  PackLanes m = {};
  int t[N0][WAVE] = {};
  for (int k = 0; k < N0; ++k)
    for (int i = 0; i < WAVE; ++i) t[k][i] = k;
  int n = N0;
  auto stage = [&](auto part, auto second) {
    for (int p = 0; p < n / 2; ++p) {
      int out[WAVE] = {};
      for (int i = 0; i < WAVE; ++i) {
        out[i] = second(i) ? t[2 * p + 1][i] : t[2 * p][i];
        if ((second(i) ? t[2 * p + 1][part(i)] : t[2 * p][part(i)]) != out[i]) return false;
      }
      for (int i = 0; i < WAVE; ++i) t[p][i] = out[i];
    }
    if (n & 1)
      for (int i = 0; i < WAVE; ++i) {
        if (t[n - 1][part(i)] != t[n - 1][i]) return false;
        t[n / 2][i] = t[n - 1][i];
      }
    n = (n + 1) / 2;
    return true;
  };
  m.ok = stage(PackStage<8>::partner, PackStage<8>::second) && stage(PackStage<4>::partner, PackStage<4>::second) &&
         stage(PackStage<2>::partner, PackStage<2>::second) && stage(PackStage<1>::partner, PackStage<1>::second) &&
         stage(PackStage<32>::partner, PackStage<32>::second) && stage(PackStage<16>::partner, PackStage<16>::second) && n == 1;
  uint64_t seen = 0;  // (4 NM <= 64 values)
  for (int i = 0; i < WAVE; ++i) {
    const int val = t[0][i];
    m.value[i] = val;
    if (val < 0 || val >= N0) {
      m.ok = false;
      continue;
    }
    if (!((seen >> val) & 1ull)) m.adds |= 1ull << i;
    seen |= 1ull << val;
    for (int b = 0; b < 4; ++b) m.term_bit[b] |= (uint64_t)(((val / GROUP) >> b) & 1) << i;
    for (int b = 0; b < 2; ++b) m.entry_bit[b] |= (uint64_t)(((val % GROUP) >> b) & 1) << i;
  }
  m.ok = m.ok && seen == (N0 == 64 ? ~0ull : (1ull << N0) - 1ull) && __builtin_popcountll(m.adds) == N0;
  return m;
}
static_assert(pack_lanes<9>().ok && pack_lanes<10>().ok && pack_lanes<11>().ok && pack_lanes<12>().ok && pack_lanes<13>().ok,
              "every moment of every entry, for every K7 row width, reaches a lane");
static_assert(pack_lanes<9>().value[0] == 0 && pack_lanes<9>().value[8] == 1 && pack_lanes<9>().value[4] == 2 &&
                  pack_lanes<9>().value[2] == GROUP && pack_lanes<9>().value[16] == 8 * GROUP,
              "nine moments: lane bits 3, 2 pick the entry, bits 1, 0, 5 the moment 0 .. 7, bit 4 the ninth");

struct Entry {
  uint32_t id;
  float4 r0, r1, r2;
};

// Can the alpha >= 1/255 level set of an entry reach the pixel rectangle [qx0, qx0 + qw] x [qy0, qy0 + qh]?  Conservative:
// `false` only if every pixel of the rectangle would take `alpha < 1/255 -> continue` (forward.cu:340-344) anyway.
// The level set is the ellipse {d : d^T Q d <= tau2}, tau2 = 2 ln(255 o), d = pixel - mean.  The test is exact up to its
// margins: the minimum of the convex form d^T Q d over the rectangle is attained on one of the two sides that face the
// mean (or is 0 when the mean lies inside), so with (cx, cy) the mean clamped into the rectangle it is
//     min( min_x q(x, cy), min_y q(cx, y) ),   min_x q(x, cy) at x = clamp(-Q_xy cy / Q_xx)  (and likewise for y).
// A misplaced minimiser only makes the value larger by a second-order amount.  (Round 1/2 bounded the ellipse by its
// axis-aligned box instead; on the headline scene 14 % of the (quadrant, entry) pairs that passed that box are rejected
// here, tools/cull_study.py, and each rejected pair saves ~40 wave instructions in the forward and ~90 in the backward.)
// Rounding: det Q = Q_xx Q_zz - Q_xy^2 cancels for a needle that is not axis aligned, and both this function's and the
// blend loops' evaluation of the form carry errors of relative size ~1e-7 against terms that are up to 2/rho times larger
// than the result (rho = det Q / (Q_xx Q_zz)).  So the test is trusted only for rho >= 1e-3, where these stay below the
// margins applied (tau2 x 1.001 + 0.02 for the exponent the loops evaluate, x 1.001 again for the value computed here,
// the rectangle widened by 0.01 pixel); worse-conditioned entries are never culled (tools/cull_replay.py replays this
// arithmetic in binary32 against the reference's per-pixel evaluation).
__device__ __forceinline__ bool can_touch_quad(const float4& r0, const float4& r1, float qx0, float qy0,
                                               float qw = (float)(QUAD - 1), float qh = (float)(QUAD - 1)) {
  // r0 = conic.x, conic.y, conic.z, opacity; r1 = mean.x, mean.y, depth, radius
  const float o = r0.w;
  if (!(o >= 1.0f / 255.0f)) return !(o == o) ? true : false;  // o < 1/255: alpha < 1/255 everywhere (NaN: keep)
  const float A = r0.x, B = r0.y, C = r0.z;
  const float xz = A * C;
  const float det = xz - B * B;
  if (!(det >= 1e-3f * xz) || !(det > 0.0f) || !(A > 0.0f)) return true;  // ill-conditioned / degenerate / NaN: never cull
  const float tau2 = 2.0f * (__logf(255.0f * o) * 1.001f + 0.01f) * 1.001f;
  const float xl = (qx0 - 0.01f) - r1.x, xh = (qx0 + qw + 0.01f) - r1.x;
  const float yl = (qy0 - 0.01f) - r1.y, yh = (qy0 + qh + 0.01f) - r1.y;
  const float cx = __builtin_amdgcn_fmed3f(0.0f, xl, xh), cy = __builtin_amdgcn_fmed3f(0.0f, yl, yh);
  const float x1 = __builtin_amdgcn_fmed3f(-(B * cy) * __builtin_amdgcn_rcpf(A), xl, xh);
  const float y2 = __builtin_amdgcn_fmed3f(-(B * cx) * __builtin_amdgcn_rcpf(C), yl, yh);
  const float q1 = (A * x1) * x1 + ((2.0f * B) * x1) * cy + (C * cy) * cy;
  const float q2 = (A * cx) * cx + ((2.0f * B) * cx) * y2 + (C * y2) * y2;
  return !(q1 > tau2) || !(q2 > tau2);  // culled only if both candidates are outside (NaN anywhere: keep)
}

// The cull rectangle of a chunk: the bounding box of the pixels of the wave that can still use an entry (`live`: not
// saturated / not yet past their last contributor), in pixel coordinates, from the 8x8 lane grid whose origin is (ox, oy).
// A long item typically ends with a few stragglers among its 64 pixels; entries that cannot reach THEM are skipped by every
// lane that still matters (on the headline scene the twenty longest forward items evaluate a third fewer entries,
// tools/cull_study.py).  Scalar arithmetic on the ballot mask: row r of the grid is byte r of the mask.
struct LiveBox {
  float x0, y0, w, h;
};
__device__ __forceinline__ LiveBox live_pixel_box(uint64_t live_mask, float ox, float oy) {
  const uint32_t ymin = (uint32_t)__builtin_ctzll(live_mask) >> 3, ymax = (63u - (uint32_t)__builtin_clzll(live_mask)) >> 3;
  uint32_t c = (uint32_t)live_mask | (uint32_t)(live_mask >> 32);
  c |= c >> 16;
  c |= c >> 8;
  c &= 0xffu;
  const uint32_t xmin = (uint32_t)__builtin_ctz(c), xmax = 31u - (uint32_t)__builtin_clz(c);
  return {ox + (float)xmin, oy + (float)ymin, (float)(xmax - xmin), (float)(ymax - ymin)};
}

// exp(power) of the blend loops: the exactly specified polynomial (bit-identical to the CPU oracle), or -- per-call
// opt-in GSR_FLAG_FAST_EXP -- the hardware's 2^x on power * log2(e) (one multiply + one quarter-rate v_exp_f32 instead
// of 12 full-rate instructions).
template <bool FAST>
__device__ __forceinline__ float blend_exp(float power) {
  if (FAST) return __builtin_amdgcn_exp2f(power * 0x1.715476p+0f);
  return gsr_expf_noclamp(power);
}

// The same for two entries at once (packed binary32: v_pk_mul / v_pk_add / v_pk_fma_f32 round each half exactly as the
// scalar instructions do; v_rndne, v_cvt and v_ldexp have no packed form and run per half).
template <bool FAST>
__device__ __forceinline__ f32x2 blend_exp2(f32x2 power) {
  const f32x2 t = power * f32x2{0x1.715476p+0f, 0x1.715476p+0f};
  if (FAST) return f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
  const f32x2 n = {__builtin_rintf(t.x), __builtin_rintf(t.y)};
  const f32x2 f = t - n;
  f32x2 p = {0x1.44138ap-13f, 0x1.44138ap-13f};
  p = __builtin_elementwise_fma(p, f, f32x2{0x1.5f0890p-10f, 0x1.5f0890p-10f});
  p = __builtin_elementwise_fma(p, f, f32x2{0x1.3b2a54p-7f, 0x1.3b2a54p-7f});
  p = __builtin_elementwise_fma(p, f, f32x2{0x1.c6af6cp-5f, 0x1.c6af6cp-5f});
  p = __builtin_elementwise_fma(p, f, f32x2{0x1.ebfbe0p-3f, 0x1.ebfbe0p-3f});
  p = __builtin_elementwise_fma(p, f, f32x2{0x1.62e430p-1f, 0x1.62e430p-1f});
  p = __builtin_elementwise_fma(p, f, f32x2{1.0f, 1.0f});
  return f32x2{__builtin_amdgcn_ldexpf(p.x, (int)n.x), __builtin_amdgcn_ldexpf(p.y, (int)n.y)};
}

// Walks list positions in chunks.  FORWARD: positions [0,len) ascending, lane l of chunk c holds
// position 64c + l.  Otherwise descending from `top`: lane l of chunk c holds top-1-(64c+l).
template <bool FORWARD, bool AUX = false>  // AUX: colours come from BlendArgs::colors3 (auxiliary forward render)
struct ChunkWalker {
  const BlendArgs& a;
  uint32_t list_base;  // range.x
  uint32_t count;      // number of positions to walk
  uint32_t id_next, id_next2;
  Entry cur, nxt;
  uint32_t chunk;  // index of the chunk held in `cur`

  __device__ __forceinline__ uint32_t pos_of(uint32_t k) const {  // k = 64*chunk + lane
    return FORWARD ? k : (count - 1 - k);
  }
  // All loads are UNCONDITIONAL (out-of-range lanes re-read the last entry): a predicated load would
  // make hipcc merge old and new register values right after the issue and wait for the data there,
  // which defeats the prefetch.
  __device__ __forceinline__ uint32_t load_id(uint32_t k) const {
    return a.point_list[list_base + pos_of(min(k, count - 1u))];
  }
  __device__ __forceinline__ void gather(Entry& e, uint32_t id) const {
    e.id = id;
    e.r0 = a.rec0[id];
    e.r1 = a.rec1[id];
    if (AUX) {  // a compile-time switch: a run-time test here costs the main kernel 8 % (measured)
      const float* __restrict__ c = a.colors3 + 3 * (size_t)id;
      e.r2 = make_float4(c[0], c[1], c[2], 0.f);
    } else {
      e.r2 = a.rec2[id];
    }
  }
  __device__ __forceinline__ ChunkWalker(const BlendArgs& a_, uint32_t base, uint32_t n) : a(a_), list_base(base), count(n) {
    const uint32_t l = (uint32_t)lane_id();
    const uint32_t id0 = load_id(l);
    id_next = load_id(WAVE + l);
    id_next2 = load_id(2 * WAVE + l);
    gather(cur, id0);
    gather(nxt, id_next);
    chunk = 0;
  }
  // number of list positions covered by the current chunk
  __device__ __forceinline__ uint32_t chunk_size() const { return min((uint32_t)WAVE, count - chunk * WAVE); }
  __device__ __forceinline__ bool valid() const { return chunk * WAVE < count; }
  // list position (0-based, in tile order) held by this lane in the current chunk
  __device__ __forceinline__ uint32_t lane_pos() const { return pos_of(chunk * WAVE + (uint32_t)lane_id()); }
  // advance: cur <- nxt, start the loads for the chunk after next
  __device__ __forceinline__ void advance() {
    const uint32_t l = (uint32_t)lane_id();
    cur = nxt;
    chunk++;
    gather(nxt, id_next2);
    id_next = id_next2;
    id_next2 = load_id((chunk + 2) * WAVE + l);
  }
};

// ---- Shared traversal pieces: chunk_cull (all five blend kernels), pair_alpha (K6, K12, the feature forward), the walk ----
// The chunk's cull test: may this lane's entry `e` of the chunk (`in_chunk`: the lane holds one the item walks) reach the
// bounding box of the pixels that are still live (`live_m`, not 0; (ox, oy): origin of the wave's 8x8 lane grid)?
__device__ __forceinline__ bool chunk_cull(uint64_t live_m, float ox, float oy, bool in_chunk, const Entry& e) {
  const LiveBox lb = live_pixel_box(live_m, ox, oy);
  return in_chunk && can_touch_quad(e.r0, e.r1, lb.x0, lb.y0, lb.w, lb.h);
}
// From the 12 geometry floats of a staged pair -- q0, q1, q2 = {hA0,hA1,nB0,nB1} {hC0,hC1,op0,op1} {x0,x1,y0,y1}, conic pre-scaled:
// (-0.5 A, -B, -0.5 C), exact; K6's FWD_PAIR begins with them --: alpha of both entries for the pixel, ZERO where the pixel skips
// the entry (power > 0 or alpha < 1/255), so that 1 - alpha = 1 and T (1 - alpha) = T exactly, and 1 - alpha.
// blend_power_prescaled and the exponential on both entries at once (packed binary32, the scalar forms' roundings).
// (The float4s BY VALUE: with `const float4&` parameters every K6 instantiation came out differently.)
constexpr int PAIR_GEOM = 12;
template <bool FAST>
__device__ __forceinline__ void pair_alpha(const float4 q0, const float4 q1, const float4 q2, const f32x2 pfx2, const f32x2 pfy2,
                                           float* ae, float* om) {
  const f32x2 hA = {q0.x, q0.y}, nB = {q0.z, q0.w}, hC = {q1.x, q1.y}, op = {q1.z, q1.w};
  const f32x2 dx = f32x2{q2.x, q2.y} - pfx2, dy = f32x2{q2.z, q2.w} - pfy2;
  const f32x2 a_ = (hA * dx) * dx;
  const f32x2 s_ = __builtin_elementwise_fma(hC * dy, dy, a_);
  const f32x2 power = __builtin_elementwise_fma(nB * dx, dy, s_);
  const f32x2 ao = op * blend_exp2<FAST>(power);
  const float a0 = fminf(0.99f, ao.x), a1 = fminf(0.99f, ao.y);
  const float g0 = (power.x > 0.0f) ? 0.0f : a0, g1 = (power.y > 0.0f) ? 0.0f : a1;
  const f32x2 a2 = {(g0 < 1.0f / 255.0f) ? 0.0f : g0, (g1 < 1.0f / 255.0f) ? 0.0f : g1};
  const f32x2 o2 = f32x2{1.0f, 1.0f} - a2;
  ae[0] = a2.x;
  ae[1] = a2.y;
  om[0] = o2.x;
  om[1] = o2.y;
}
// K12 and the feature forward: ONE walk over an item's list, front to back -- ChunkWalker, the cull against the live pixels'
// box, survivors compacted in order and staged in pairs of PAIR_GEOM floats (the caller's `stage(slot, entry)` adds its
// payload: an id, a feature row), four survivors per iteration evaluated two per packed instruction, the serial part on
// selects as in K6's fast path: Ts = T for a live pixel, -T for one that is done.
//   entry skipped for this pixel (ae = 0, om = 1): test_T = T exactly, no hit;
//   T (1 - alpha) < 0.0001: the pixel is done BEFORE this entry counts (forward.cu:349-354, apply_weights.cu:318-323), Ts := -T;
//   pixel done: test_T <= 0, nothing changes.
// Per evaluated group `group(j, hit, w)` gets, for the entries j .. j + 3 of the chunk's survivors, whether this lane's pixel
// blends the entry and, where it does, its weight alpha T (two arrays: K12 never forms the weights -- as the sign of one masked
// weight array the test cost its groups four multiplies and selects); behind the chunk's groups `chunk_end(n)` gets the number of survivors whose groups
// were evaluated (all of them unless every pixel saturated on the way).  (Rounds 1-5 of K12 walked one survivor per iteration
// with a ballot, a branch and a 64-lane reduction per entry: 182 -> 122 us per 512 x 512 view at 10^6 Gaussians,
// profiles/r06_j_trace_weights.md.)  One-wave workgroups: the barriers around the staging are free.
template <bool FAST, class Stage, class Group, class ChunkEnd>
__device__ __forceinline__ void walk_front_to_back(const BlendArgs& a, const PixelWave& pw, const uint2 range, Stage&& stage,
                                                   Group&& group, ChunkEnd&& chunk_end) {
  __shared__ __align__(16) float spair[WAVE / 2][PAIR_GEOM];
  if (range.y <= range.x) return;
  const int lane = lane_id();
  const float pfx = (float)pw.px, pfy = (float)pw.py;
  const f32x2 pfx2 = {pfx, pfx}, pfy2 = {pfy, pfy};
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  float Ts = pw.inside ? 1.0f : -1.0f;
  ChunkWalker<true> walk(a, range.x, range.y - range.x);
  for (; walk.valid(); walk.advance()) {
    const uint64_t live_m = __ballot(Ts > 0.0f);
    if (live_m == 0) break;
    const bool keep = chunk_cull(live_m, pfx - (float)(lane & 7), pfy - (float)(lane >> 3), (uint32_t)lane < walk.chunk_size(), walk.cur);
    const uint64_t km = __ballot(keep);
    if (km == 0) continue;
    const uint32_t n = (uint32_t)__popcll(km);
    const uint32_t n4 = (n + GROUP - 1) & ~(uint32_t)(GROUP - 1);
    __syncthreads();
    if (keep) {
      const uint32_t slot = (uint32_t)__popcll(km & lt_mask);
      float* q = &spair[slot >> 1][slot & 1u];
      q[0] = -0.5f * walk.cur.r0.x;
      q[2] = -walk.cur.r0.y;
      q[4] = -0.5f * walk.cur.r0.z;
      q[6] = walk.cur.r0.w;
      q[8] = walk.cur.r1.x;
      q[10] = walk.cur.r1.y;
      stage(slot, walk.cur);
    }
    if ((uint32_t)lane >= n && (uint32_t)lane < n4) {
      // null entries pad the survivors to a multiple of GROUP: opacity 0 => alpha 0 => never a hit
      float* q = &spair[lane >> 1][lane & 1];
      q[0] = q[2] = q[4] = q[6] = q[8] = q[10] = 0.f;
    }
    __syncthreads();
    uint32_t evaluated = n;  // survivors whose groups were evaluated (all of them unless every pixel saturated on the way)
    for (uint32_t j = 0; j < n4; j += GROUP) {
      if (__all(Ts < 0.0f)) {
        evaluated = j;
        break;
      }
      float ae[GROUP], om[GROUP], w[GROUP];
      bool hit[GROUP];
#pragma unroll
      for (int pp = 0; pp < GROUP / 2; ++pp) {
        const float* q = &spair[(j >> 1) + pp][0];
        pair_alpha<FAST>(*reinterpret_cast<const float4*>(q), *reinterpret_cast<const float4*>(q + 4),
                         *reinterpret_cast<const float4*>(q + 8), pfx2, pfy2, ae + 2 * pp, om + 2 * pp);
      }
      // (the four footprints pinned ahead of the serial part, as in K6)
#pragma unroll
      for (int u = 0; u < GROUP; ++u) asm volatile("" : "+v"(ae[u]), "+v"(om[u]));
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        const float test_T = Ts * om[u];
        const bool A = !(test_T < 0.0001f);
        hit[u] = A && ae[u] > 0.0f;
        w[u] = ae[u] * Ts;
        Ts = A ? test_T : -__builtin_fabsf(Ts);
      }
      group(j, hit, w);
    }
    chunk_end(min(n, evaluated));
  }
}

// ----------------------------------------------------------------------------------
// K6: renderCUDA (forward), DGR/cuda_rasterizer/forward.cu:261-379.
// ----------------------------------------------------------------------------------
// One forward item: a quadrant of `tile` (or, on small images, a part of one: SPLIT).  `bg0..2`: the background, read once
// per kernel into scalar registers (see blend_forward_kernel).
template <bool PROFILE, bool AUX, int SPLIT, bool FAST, bool CKPT>
__device__ __forceinline__ void forward_item(const BlendArgs& a, uint32_t tile, uint32_t quad, const float bg0, const float bg1,
                                             const float bg2, uint32_t& prof_visited, uint64_t* prof_cyc) {
  PixelWave pw;
  ItemBox box;
  if (!setup_item<SPLIT>(a, tile, quad, pw, box)) return;  // (work_est / work_maxc were cleared by tile_worklist_kernel)
  quad &= 3u;
  const int lane = lane_id();
  const uint2 range = a.ranges[pw.tile];
  const float pfx = (float)pw.px, pfy = (float)pw.py;
  (void)box;  // (the cull rectangle follows the pixels that are still live, live_pixel_box)
  bool done = !pw.inside;
  float T = 1.0f;
  uint32_t last_contributor = 0;
  uint32_t evaluated = 0;  // entries this quadrant evaluated (wave-uniform): the backward's work estimate for the tile

  // Staging layout: the survivors of a chunk are stored in PAIRS, the two entries' values of each footprint input next
  // to each other, so that one uniform ds_read_b128 puts them into adjacent registers and the footprint arithmetic of
  // two entries runs as packed binary32 instructions (v_pk_add / v_pk_mul / v_pk_fma_f32: two IEEE operations per lane
  // and issue slot, the same roundings as the scalar forms).  A wave issues at most one instruction every four cycles,
  // and the forward ends with its longest item, so the instruction count of an entry is what the kernel's length follows.
  //   pair p (entries 2p, 2p+1), FWD_PAIR floats: [0] hA0 hA1 nB0 nB1 | [4] hC0 hC1 op0 op1 | [8] x0 x1 y0 y1 |
  //                                               [12] r0 g0 b0 z0 | [16] r1 g1 b1 z1 | [20] pos0 pos1 - -
  constexpr int FWD_PAIR = 24;
  __shared__ __attribute__((aligned(16))) float sp[(WAVE / 2) * FWD_PAIR];
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  const f32x2 pfx2 = {pfx, pfx}, pfy2 = {pfy, pfy};
  f32x2 C01 = {0.f, 0.f}, C2D = {0.f, 0.f};  // (C0, C1), (C2, D)
  // CKPT: the colour accumulated SINCE THE LAST CHECKPOINT, in accumulators of its own (round 5).  The backward needs, at a
  // segment's upper end, the colour of everything behind it; as C_final - C(checkpoint) that is a difference of two sums
  // near 1 whose increments were rounded to 6e-8 each, divided by a transmittance that may be 0.01 -- the gradients of a
  // Gaussian in front of a dense segment came out 1e-5 .. 2e-5 off (tools/fuzz_v2.py, seed 365).  A segment's own sum
  // carries its own magnitude's rounding only.
  f32x2 S01 = {0.f, 0.f};
  float S2 = 0.f;
  // Checkpoints for the backward's list segments (Image::ck_*): in front of list position pos(k) (CkTable) the state of every
  // pixel that is still live -- transmittance and accumulated colour -- goes into the tile's slot k (one 16-byte store per
  // lane and one atomic per wave: the slots are assigned by tile_worklist_kernel, nothing is allocated here).
  // (CKPT: a template switch, chosen per view by the host -- views with short lists run the kernel without any of this)
  constexpr bool ckpt = CKPT && !AUX;
  const uint32_t pidx = (uint32_t)((pw.py & (TILE - 1)) * TILE + (pw.px & (TILE - 1)));  // pixel inside its tile
  const uint32_t ck_base = ckpt ? a.ck_table[tile] : CK_NONE;  // rank of the tile among the checkpointed ones
  uint32_t ck_next = (ckpt && ck_base != CK_NONE) ? (uint32_t)a.ck_pos.chunk[1] : 0xffffffffu, ck_k = 1u;
  auto stage = [&](uint32_t slot, float hA, float nB, float hC, float op, float x, float y, float z, float r, float g,
                   float b, float pos) {
    float* q = sp + (slot >> 1) * FWD_PAIR + (slot & 1u);
    q[0] = hA;
    q[2] = nB;
    q[4] = hC;
    q[6] = op;
    q[8] = x;
    q[10] = y;
    q[20] = pos;
    *reinterpret_cast<float4*>(sp + (slot >> 1) * FWD_PAIR + 12 + 4 * (slot & 1u)) = make_float4(r, g, b, z);
  };
  if (range.y > range.x) {
    ChunkWalker<true, AUX> walk(a, range.x, range.y - range.x);
    for (; walk.valid(); walk.advance()) {
      const uint64_t live_m = __ballot(!done);
      if (live_m == 0) break;
      if (ckpt && walk.chunk == ck_next) {  // (uniform; never for walks shorter than the stride)
        if (ck_k < (uint32_t)a.ck_slots) {
          // slot k: T in front of position pos(k), and the colour of segment k - 1.  Written by every pixel of the
          // quadrant (a saturated one writes zeros: the backward never reads them, but it may read the slots of a pixel that
          // is live and simply found nothing to blend)
          if (pw.inside) a.ck_pool[((size_t)ck_base * (uint32_t)a.ck_slots + ck_k) * (TILE * TILE) + pidx] = make_float4(T, S01.x, S01.y, S2);
          S01 = f32x2{0.f, 0.f};
          S2 = 0.f;
          // (what this wave has evaluated so far: the backward's work list splits the tile's estimate with it)
          if (lane == 0) atomicAdd(&a.ck_work[(size_t)tile * (uint32_t)a.ck_slots + ck_k], evaluated);
        }
        ck_k++;
        ck_next = ck_k < (uint32_t)a.ck_slots ? (uint32_t)a.ck_pos.chunk[ck_k] : 0xffffffffu;  // (the table is ascending)
      }
      uint64_t tc0 = 0;
      if (PROFILE) {
        tc0 = __builtin_amdgcn_s_memtime();
        prof_cyc[2]++;  // chunks walked
      }
      const bool keep = chunk_cull(live_m, pfx - (float)(lane & 7), pfy - (float)(lane >> 3), (uint32_t)lane < walk.chunk_size(), walk.cur);
      const uint64_t m = __ballot(keep);
      if (PROFILE) prof_cyc[3] += __builtin_amdgcn_s_memtime() - tc0;  // wait for the chunk's records + cull
      if (m == 0) continue;
      const uint32_t cnt = (uint32_t)__popcll(m);
      const uint32_t cnt4 = (cnt + GROUP - 1) & ~(uint32_t)(GROUP - 1);
      __syncthreads();
      // a staged colour or depth that is NaN / Inf (0 * c would no longer be 0): this chunk takes the masked form
      const float csum = (walk.cur.r2.x + walk.cur.r2.y) + (walk.cur.r2.z + walk.cur.r1.z);
      const bool bad_value = keep && !(csum - csum == 0.0f);
      if (keep)  // conic pre-scaled: (-0.5 A, -B, -0.5 C), exact
        stage((uint32_t)__popcll(m & lt_mask), -0.5f * walk.cur.r0.x, -walk.cur.r0.y, -0.5f * walk.cur.r0.z, walk.cur.r0.w,
              walk.cur.r1.x, walk.cur.r1.y, walk.cur.r1.z, walk.cur.r2.x, walk.cur.r2.y, walk.cur.r2.z,
              __uint_as_float(walk.lane_pos() + 1u));
      if ((uint32_t)lane >= cnt && (uint32_t)lane < cnt4)
        // null entries pad the survivors to a multiple of GROUP: opacity 0 => alpha 0 => never a hit
        stage((uint32_t)lane, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
      __syncthreads();
      // GROUP entries per iteration: the footprint / exp evaluations of a group are independent
      // straight-line code (ILP for a wave that is alone on its SIMD); only the short
      // transmittance chain below is serial.
      uint64_t tc1 = 0;
      if (PROFILE) {
        tc1 = __builtin_amdgcn_s_memtime();
        prof_cyc[0] += tc1 - tc0;  // chunk start -> staged
      }
      if (!__any(bad_value)) {
        // Fast path (every staged colour / depth of the chunk is finite): the serial part runs on selects only, in one
        // basic block without a single scalar instruction.  A wave issues one instruction about every 4.7 cycles whatever
        // its type, and a v_cmp -> SALU -> exec -> VALU turn costs ~40 cycles against ~13 for v_mul -> v_cmp -> v_cndmask
        // (tools/microbench/issue_rate.hip), so the length of the longest item follows the instruction count and the
        // number of such turns.  State: Ts = T for a live lane, -T for one that is done (out of the image, or saturated).
        //   entry skipped for this pixel (power > 0 or alpha < 1/255): alpha := 0, so 1 - alpha = 1, test_T = T exactly,
        //     w = 0 and the accumulators take c * 0 = 0 (c finite);
        //   T (1 - alpha) < 0.0001: A is false, w := 0, Ts := -T (final_T stays the T before this entry, forward.cu:349-354);
        //   lane done: test_T <= 0 < 0.0001, A false, nothing changes.
        // Same operations and roundings as the masked form below wherever a value is kept.
        float Ts = done ? -T : T;
        for (uint32_t j = 0; j < cnt4; j += GROUP) {
          if (__all(Ts < 0.0f)) break;
          evaluated += GROUP;
          if (PROFILE) prof_visited += GROUP;
          float ae[GROUP], om[GROUP], posf[GROUP];
          f32x2 rg[GROUP], bz[GROUP];
#pragma unroll
          for (int pp = 0; pp < GROUP / 2; ++pp) {
            const float* q = sp + ((j >> 1) + pp) * FWD_PAIR;
            const float4 q0 = *reinterpret_cast<const float4*>(q), q1 = *reinterpret_cast<const float4*>(q + 4),
                         q2 = *reinterpret_cast<const float4*>(q + 8), c0 = *reinterpret_cast<const float4*>(q + 12),
                         c1 = *reinterpret_cast<const float4*>(q + 16);
            const float2 ps = *reinterpret_cast<const float2*>(q + 20);
            // (the pair's loads all stand in front of the arithmetic, in this order: with the colour loads behind it the
            //  CKPT and PROFILE kernels came out differently)
            pair_alpha<FAST>(q0, q1, q2, pfx2, pfy2, ae + 2 * pp, om + 2 * pp);
            rg[2 * pp] = f32x2{c0.x, c0.y};
            bz[2 * pp] = f32x2{c0.z, c0.w};
            rg[2 * pp + 1] = f32x2{c1.x, c1.y};
            bz[2 * pp + 1] = f32x2{c1.z, c1.w};
            posf[2 * pp] = ps.x;
            posf[2 * pp + 1] = ps.y;
          }
#pragma unroll
          for (int u = 0; u < GROUP; ++u) asm volatile("" : "+v"(ae[u]), "+v"(om[u]));
#pragma unroll
          for (int u = 0; u < GROUP; ++u) {
            // (the walk's Ts step, written out: as a helper -- by reference, a struct by value, a callback in the middle -- it
            //  moved every K6 instantiation)
            const float test_T = Ts * om[u];
            const bool A = !(test_T < 0.0001f);
            const float w = ae[u] * Ts;
            const float wz = A ? w : 0.0f;
            const f32x2 w2 = {wz, wz};
            C01 = __builtin_elementwise_fma(rg[u], w2, C01);
            C2D = __builtin_elementwise_fma(bz[u], w2, C2D);
            if (ckpt) {
              S01 = __builtin_elementwise_fma(rg[u], w2, S01);
              S2 = __builtin_fmaf(bz[u].x, wz, S2);
            }
            Ts = A ? test_T : -__builtin_fabsf(Ts);
            last_contributor = (wz > 0.0f) ? __float_as_uint(posf[u]) : last_contributor;
          }
        }
        done = Ts < 0.0f;
        T = __builtin_fabsf(Ts);
      } else {
        for (uint32_t j = 0; j < cnt4; j += GROUP) {
          if (__all(done)) break;
          evaluated += GROUP;
          if (PROFILE) prof_visited += GROUP;
          float al[GROUP], om[GROUP], posf[GROUP];
          bool ok[GROUP];
          f32x2 rg[GROUP], bz[GROUP];
  #pragma unroll
          for (int pp = 0; pp < GROUP / 2; ++pp) {
            const float* q = sp + ((j >> 1) + pp) * FWD_PAIR;
            const float4 q0 = *reinterpret_cast<const float4*>(q), q1 = *reinterpret_cast<const float4*>(q + 4),
                         q2 = *reinterpret_cast<const float4*>(q + 8), c0 = *reinterpret_cast<const float4*>(q + 12),
                         c1 = *reinterpret_cast<const float4*>(q + 16);
            const float2 ps = *reinterpret_cast<const float2*>(q + 20);
            const f32x2 hA = {q0.x, q0.y}, nB = {q0.z, q0.w}, hC = {q1.x, q1.y}, op = {q1.z, q1.w};
            const f32x2 dx = f32x2{q2.x, q2.y} - pfx2, dy = f32x2{q2.z, q2.w} - pfy2;
            // blend_power_prescaled on both entries
            const f32x2 a_ = (hA * dx) * dx;
            const f32x2 s_ = __builtin_elementwise_fma(hC * dy, dy, a_);
            const f32x2 power = __builtin_elementwise_fma(nB * dx, dy, s_);
            const f32x2 e = blend_exp2<FAST>(power);
            const f32x2 ao = op * e;
            const f32x2 a2 = {fminf(0.99f, ao.x), fminf(0.99f, ao.y)};
            const f32x2 o2 = f32x2{1.0f, 1.0f} - a2;
            al[2 * pp] = a2.x;
            al[2 * pp + 1] = a2.y;
            om[2 * pp] = o2.x;
            om[2 * pp + 1] = o2.y;
            ok[2 * pp] = !(power.x > 0.0f) && !(a2.x < 1.0f / 255.0f);
            ok[2 * pp + 1] = !(power.y > 0.0f) && !(a2.y < 1.0f / 255.0f);
            rg[2 * pp] = f32x2{c0.x, c0.y};
            bz[2 * pp] = f32x2{c0.z, c0.w};
            rg[2 * pp + 1] = f32x2{c1.x, c1.y};
            bz[2 * pp + 1] = f32x2{c1.z, c1.w};
            posf[2 * pp] = ps.x;
            posf[2 * pp + 1] = ps.y;
          }
          // pin the four footprints ahead of the serial part: otherwise the optimiser sinks each one into the masked
          // region that consumes it and the independent exp chains no longer overlap (forward blend -2 %)
  #pragma unroll
          for (int u = 0; u < GROUP; ++u) asm volatile("" : "+v"(al[u]), "+v"(om[u]));
  #pragma unroll
          for (int u = 0; u < GROUP; ++u) {
            const bool hit = ok[u] && !done;
            const float test_T = T * om[u];
            const bool term = hit && (test_T < 0.0001f);
            done = done || term;
            if (hit && !term) {  // kept as a lane-masked region: fewer instructions under exec than selects
              const float w = al[u] * T;
              const f32x2 w2 = {w, w};
              C01 = __builtin_elementwise_fma(rg[u], w2, C01);
              C2D = __builtin_elementwise_fma(bz[u], w2, C2D);
              if (ckpt) {
                S01 = __builtin_elementwise_fma(rg[u], w2, S01);
                S2 = __builtin_fmaf(bz[u].x, w, S2);
              }
              T = test_T;
              last_contributor = __float_as_uint(posf[u]);
            }
          }
        }
      }
      if (PROFILE) prof_cyc[1] += __builtin_amdgcn_s_memtime() - tc1;  // group loop
    }
  }
  const float C0 = C01.x, C1 = C01.y, C2 = C2D.x, D = C2D.y;
  // how deep the backward will walk this quadrant's part of the list (a lane outside the image never contributes)
  const uint32_t deep = (a.work_est != nullptr || ckpt) ? wave_max_u32_dpp(last_contributor) : 0u;
  if (ckpt) {
    // ... for the whole tile, and -- for the pixels some checkpoint was written for -- the colour of the segment the walk
    // ended in, as if its closing checkpoint had been reached: slot ck_k, or slot 0 once the tile's slots are used up (that
    // "segment" then reaches to the end of the list).  With it the colour of segment k is ALWAYS in slot k + 1 (k + 1 < ck_slots)
    // or in slot 0 (k = ck_slots - 1), whether the wave went on beyond it or not.
    if (deep > a.ck_pos.pos(1u) && lane == 0) atomicMax(&a.tile_maxc[tile], deep);
    if (ck_k > 1u && pw.inside)
      a.ck_pool[((size_t)ck_base * (uint32_t)a.ck_slots + (ck_k < (uint32_t)a.ck_slots ? ck_k : 0u)) * (TILE * TILE) + pidx] = make_float4(T, S01.x, S01.y, S2);
  }
  // the backward's work estimate and walk depth for the quadrant.  One item per quadrant: plain stores; the sub-items of a
  // cut quadrant report the largest of their values (they walk the same list; their SUM as the estimate was measured and is
  // worse, profiles/r06_s_forward_split.md).
  if (a.work_est != nullptr && lane == 0) {
    if (SPLIT == 1) {
      a.work_est[4u * tile + quad] = evaluated;
      a.work_maxc[4u * tile + quad] = deep;
    } else {
      atomicMax(&a.work_est[4u * tile + quad], evaluated);
      atomicMax(&a.work_maxc[4u * tile + quad], deep);
    }
  }
  if (pw.inside) {
    const size_t pix = (size_t)pw.py * a.W + pw.px, HW = (size_t)a.H * a.W;
    if (a.final_T != nullptr) {  // (null in an auxiliary render: the state the backward needs stays that of the main one)
      a.final_T[pix] = T;
      a.n_contrib[pix] = last_contributor;
    }
    a.out_color[pix] = __builtin_fmaf(T, bg0, C0);
    a.out_color[HW + pix] = __builtin_fmaf(T, bg1, C1);
    a.out_color[2 * HW + pix] = __builtin_fmaf(T, bg2, C2);
    if (a.out_depth != nullptr) a.out_depth[pix] = D;
  }
}

template <bool PROFILE, bool AUX, int SPLIT, bool FAST, bool CKPT>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4))) blend_forward_kernel(const BlendArgs a) {
  uint64_t t_start = 0;
  uint32_t prof_visited = 0, prof_items = 0;
  uint64_t prof_cyc[4] = {0, 0, 0, 0};
  if (PROFILE) t_start = __builtin_amdgcn_s_memtime();
  const float bg0 = wave_uniform(a.bg[0]), bg1 = wave_uniform(a.bg[1]), bg2 = wave_uniform(a.bg[2]);
  // (always_inline: past a size threshold hipcc stops inlining the item function into the work loop's two call sites and
  //  CALLS it -- the 300-byte argument block then travels through scratch memory)
  run_work_queue<SPLIT>(a, true, [&](uint32_t tile, uint32_t quad, bool empty) __attribute__((always_inline)) {
    if (PROFILE) prof_items++;
    if (!empty) {
      forward_item<PROFILE, AUX, SPLIT, FAST, CKPT>(a, tile, quad, bg0, bg1, bg2, prof_visited, prof_cyc);
    } else {
      // a tile no Gaussian touches: background only (forward.cu:371-378 with an empty range)
      for_each_pixel_of_tile(a, tile, [&](size_t pix, size_t HW) __attribute__((always_inline)) {
        if (a.final_T != nullptr) {
          a.final_T[pix] = 1.0f;
          a.n_contrib[pix] = 0u;
        }
        a.out_color[pix] = __builtin_fmaf(1.0f, bg0, 0.f);
        a.out_color[HW + pix] = __builtin_fmaf(1.0f, bg1, 0.f);
        a.out_color[2 * HW + pix] = __builtin_fmaf(1.0f, bg2, 0.f);
        if (a.out_depth != nullptr) a.out_depth[pix] = 0.f;
      });
    }
  });
  if (PROFILE) {
    // debug record per persistent wave (8 x u64): start, end (s_memtime ticks), XCC_ID<<32 | HW_ID,
    // items<<32 | visited entries, then the cycle split below
    const uint64_t t_end = __builtin_amdgcn_s_memtime();
    if (lane_id() == 0) {
      uint64_t* rec = a.profile + (size_t)blockIdx.x * 8;
      rec[4] = prof_cyc[0];  // cycles: chunk start -> survivors staged
      rec[5] = prof_cyc[1];  // cycles: group loops
      rec[6] = prof_cyc[2];  // chunks walked
      rec[7] = prof_cyc[3];  // cycles: chunk start -> cull ballot (includes the wait for the gathered records)
      rec[0] = t_start;
      rec[1] = t_end;
      rec[2] = ((uint64_t)xcc_id() << 32) | (uint64_t)__builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4);  // HW_REG_HW_ID
      rec[3] = ((uint64_t)prof_items << 32) | (uint64_t)prof_visited;
    }
  }
}

// ----------------------------------------------------------------------------------
// K7: renderCUDA (backward), DGR/cuda_rasterizer/backward.cu:399-557.
// ----------------------------------------------------------------------------------
// Wave-level ordering of LDS traffic inside a multi-wave workgroup: a wave runs in lockstep, so all
// that is needed is that the compiler keeps program order and waits for the LDS queue.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

constexpr int BWD_WAVES = 4;  // one workgroup = the four quadrants of one tile (or two quadrants of a heavy one)
constexpr int ACC_LDS_ROW = 9;  // floats per chunk slot of the backward's LDS accumulators: the nine raw moments
// ... of a DEPTH backward (gsr_blend_backward_depth): ten raw moments (the tenth: alpha T dL_ddepth) in rows of 11 floats
// (odd, as 9: the rows of the tail's ds_add -- up to four slots, two per 32-lane half -- and the four rows of a flush
// instruction spread over the banks)
// ... of an ABS backward (GSR_FLAG_ABS_GRAD): two more raw moments behind those, |A qx + B qy| and |B qx + C qy|, in rows of
// 11 floats, with DEPTH 13 (odd again)
template <bool DEPTH, bool ABS = false> constexpr int bwd_moments() { return (DEPTH ? 10 : 9) + (ABS ? 2 : 0); }
template <bool DEPTH, bool ABS = false> constexpr int bwd_lds_row() { return ABS ? (DEPTH ? 13 : 11) : DEPTH ? 11 : ACC_LDS_ROW; }
constexpr uint32_t BWD_ITEM_HALF = 0x80000000u;   // item code: the workgroup handles one half of the tile ...
constexpr uint32_t BWD_ITEM_PART = 0x40000000u;   // ... quadrants {2,3} instead of {0,1}
// ... or (round 4) A RUN OF LIST SEGMENTS of a deep tile: the segments lo .. hi between its checkpoints, i.e. positions
// [pos(lo), pos(hi + 1)) of its list (CkTable: where a view's checkpoints sit), a run that ends with the tile's last segment
// up to the tile's deepest contributor.  The
// pixels that still contribute behind the run start from the forward's checkpoint in front of its upper end instead of from
// their final state (backward_tile).  The work list makes one item per stride (lo == hi): runs of several strides, merged
// to about equal measured work, were measured in round 6 and bought nothing (profiles/r06_m_fine_checkpoints.md).
constexpr uint32_t BWD_ITEM_SEG = 0x10000000u;
static_assert(BWD_ITEM_SEG == BWD_ITEM_SEG_BIT, "gsr_kernels.h states the bit gsr_debug_blend_backward_items counts");
constexpr int BWD_SEG_SHIFT = 20, BWD_NSEG_SHIFT = 24;  // 4 bits each: first stride of the run, last stride of the run
static_assert(CK_MAX <= 16, "a stride index must fit the item code's 4 bits");
constexpr uint32_t BWD_ITEM_TILE = 0x000fffffu;   // (images of up to 2^20 tiles: GSR_MAX_TILES, checked by gsr_blend_backward)
static_assert(BWD_ITEM_TILE + 1u == (uint32_t)GSR_MAX_TILES, "include/gsr.h states the backward's tile limit");

// ---- What K7 and the feature backward share: the item's descriptor and the per-entry arithmetic ----
// The item's descriptor from three SCALAR loads (tables of earlier kernels: the work list, the ranges, the walk depths the
// forward left per quadrant; the scalar path does not queue behind the previous item's last atomics): code first, the other
// two together.  x = code, y = first position of the tile's list, z = how deep the item's pixels reach into it (the forward's
// work_maxc: of the whole tile, or of the half the item covers), w = length of the tile's list.  (Round 5's first form had
// backward_worklist_kernel write whole descriptors: that one-block kernel is a chain of dependent round trips between the
// forward and the backward -- 14 -> 16-18 us for what costs this kernel, whose waves wait behind three others, nothing
// measurable.)
__device__ __forceinline__ uint4 load_backward_item(const BlendArgs& a, uint32_t index) {
  const uint32_t code = scalar_load(a.bwd_order, index);
  const uint32_t ctile = code & BWD_ITEM_TILE;
  const uint2 crange = scalar_load(a.ranges, ctile);
  const uint4 cmax = scalar_load(reinterpret_cast<const uint4*>(a.work_maxc), ctile);
  const uint32_t r01 = max(cmax.x, cmax.y), r23 = max(cmax.z, cmax.w);
  return make_uint4(code, crange.x, (code & BWD_ITEM_HALF) ? ((code & BWD_ITEM_PART) ? r23 : r01) : max(r01, r23), crange.y - crange.x);
}
// 1 / (1 - alpha) of the transmittance chain (backward.cu:503): the reciprocal refined by one Newton step.  Along a list of
// thousands of translucent entries the raw v_rcp_f32's error (1 ulp) accumulated to 1e-5 of a gradient
// (profiles/r05_d_precision_fuzz.md).
__device__ __forceinline__ float rcp_refined(float x) {
  const float r0 = __builtin_amdgcn_rcpf(x);
  return __builtin_fmaf(r0, __builtin_fmaf(-x, r0, 1.0f), r0);
}
// One entry of the collapsed colour recurrence, backward.cu:503-534: the reference keeps accum_rec[ch] and last_color[ch] per
// channel and forms sum_ch (c[ch] - accum_rec[ch]) * dL_dpixel[ch]; the recurrence is linear and dL_dpixel is constant for the
// pixel, so B = sum_ch accum_rec[ch] * dL_dpixel[ch] obeys the same recurrence with the scalar cdot = sum_ch c[ch] *
// dL_dpixel[ch] in place of the colour.  A lane that does not contribute (`on` false, alpha = 0) runs the same arithmetic: its
// transmittance is multiplied by rcp(1) = 1 exactly, the pending fold of (last_alpha, last_cdot) into B happens now instead
// of at the lane's next contributor (same operands, same value; afterwards last_alpha = 0 makes the fold a no-op) -- three
// selects per entry instead of six.  Hands back the new T and B and dL/dalpha WITHOUT the background's share (K7 adds its own);
// the caller then sets last_alpha = alpha and keeps last_cdot by a select (last_cdot = on ? cdot : last_cdot: a NaN colour of
// a skipped entry must not enter B as 0 * NaN).  State in and out BY VALUE: with `float&` parameters every K7 instantiation
// came out differently.
struct RecStep {
  float T, B_acc, dL_dalpha;
};
__device__ __forceinline__ RecStep accum_rec_step(float T, float B_acc, float last_alpha, float last_cdot, float inv_one_m, float cdot) {
#pragma clang fp contract(fast)  // gradients are tolerance-checked (<= 1e-5), not bit-compared: let a*b+c fuse here
  RecStep r;
  r.T = T * inv_one_m;                                 // T / (1 - alpha), backward.cu:503
  r.B_acc = B_acc + last_alpha * (last_cdot - B_acc);  // accum_rec update, backward.cu:515
  r.dL_dalpha = (cdot - r.B_acc) * r.T;
  return r;
}
// The six raw geometry moments of q = G dL/dalpha of entry u of a group (dx, dy: the entry's mean relative to the pixel).  Per
// lane only the MOMENTS are formed; every per-entry constant of backward.cu:538-554 (conic, opacity, 0.5*W, 0.5*H, -0.5) is
// applied once per (tile, entry) by the flush.
template <int NM>
__device__ __forceinline__ void geometry_moments(float (&v)[NM][GROUP], int u, float q, float dx, float dy) {
#pragma clang fp contract(fast)
  const float qx = q * dx, qy = q * dy;
  v[0][u] = q;
  v[1][u] = qx;
  v[2][u] = qy;
  v[3][u] = qx * dx;
  v[4][u] = qx * dy;
  v[5][u] = qy * dy;
}

// One tile, processed by a 4-wave workgroup (wave w = quadrant w).  The four waves walk the tile's list
// back to front in the SAME 64-entry chunks; each wave culls / compacts / evaluates the chunk for its own
// 64 pixels exactly as before, but the wave totals of the nine gradient terms are summed over the four
// quadrants in LDS (ds_add_f32), and only then does one global atomic per (tile, instance, term) leave
// the CU.  The global float atomics execute at the memory side on this chip and were the largest single
// cost of the backward (about 200 of 530 us with one atomic per quadrant); a Gaussian typically touches
// 2-3 of a tile's 4 quadrants.
//
// DEPTH (gsr_blend_backward_depth): the depth image D = sum_i d_i alpha_i T_i is a fourth blended channel with background 0.
// Its share of dL/dalpha_i is (d_i - depth behind) T_i dL_dD: the entry's depth (staged in s1.z) joins cdot as d_i dL_dD,
// and B_acc, which follows the same linear recurrence, then carries the depth behind as well.  The tenth raw moment
// alpha T dL_dD is dL/dd_i, flushed into column ACC_DEPTH.  No list segments (SEG): the forward's checkpoints hold the
// colour behind a segment, not its depth.
//
// ABS (GSR_FLAG_ABS_GRAD): next to the signed screen-space gradient the sum over pixels of the ABSOLUTE values of its
// per-pixel terms (backward.cu:545-546) is accumulated, into the columns ACC_ABS2D, + 1.  The per-pixel term of the x
// component is -o (A qx + B qy) 0.5 W: o, 0.5 W and 0.5 H are per-entry constants, so the lane forms |A qx + B qy| and
// |B qx + C qy| from the conic it already holds (pre-scaled: A = -2 cos_.x, B = -cos_.y, C = -2 cos_.z; the common sign
// drops out of the absolute value), the two moments are reduced and added to the chunk's LDS row like the others, and the
// flush multiplies by |o| 0.5 W, |o| 0.5 H.  Every item shape takes it as it is: an entry is seen once by every pixel of an
// item, whole tile, half tile or list segment, and absolute sums add over any partition of the pixels.
//
// ALPHA (gsr_blend_backward_alpha): the alpha image A = 1 - T_final of the pixel carries a gradient gA.  dA/dalpha_i =
// T_final / (1 - alpha_i) for every blended entry: the shape of the background's share, with the opposite sign -- so gA is
// subtracted from bg . dL_dpixel, once per pixel, and everything behind dL/dalpha moves with it (the ABS sums included).  A
// list segment takes it as it is: the term is applied per entry from the pixel's own T_final, whatever lies behind the run.
template <bool FAST, bool SEG, bool DEPTH, bool ABS, bool ALPHA>
__device__ __forceinline__ uint32_t backward_tile(const BlendArgs& a, const uint4 item, const float bg0, const float bg1,
                                              const float bg2, float4 (*s0)[WAVE], float4 (*s1)[WAVE], float4 (*s2)[WAVE],
                                              uint32_t (*sid)[WAVE], float4 (*sco)[WAVE],
                                              float (*sacc)[WAVE][bwd_lds_row<DEPTH, ABS>()]) {
  static_assert(!(DEPTH && SEG), "depth backwards walk whole lists: the checkpoints hold no depth");
  constexpr int NM = bwd_moments<DEPTH, ABS>();  // raw moments per entry
  constexpr int IABS = bwd_moments<DEPTH>();     // (ABS) index of the first of the two absolute moments
  const int w = (int)(threadIdx.x >> 6), lane = lane_id();
  // the group loop's tail (wave_sum4_pack): the moment, and the entry of the group, whose total this lane ends up with, and
  // whether it is the lane that adds it
  constexpr PackLanes tail = pack_lanes<NM>();
  auto tail_bit = [lane](uint64_t plane) __attribute__((always_inline)) { return (uint32_t)(plane >> (uint32_t)lane) & 1u; };
  const uint32_t tail_term = tail_bit(tail.term_bit[0]) | tail_bit(tail.term_bit[1]) << 1 | tail_bit(tail.term_bit[2]) << 2 |
                             tail_bit(tail.term_bit[3]) << 3;
  const uint32_t tail_entry = tail_bit(tail.entry_bit[0]) | tail_bit(tail.entry_bit[1]) << 1;
  const bool tail_adds = tail_bit(tail.adds) != 0u;
  // The item's descriptor (assembled by the caller from three scalar loads): x = code -- a whole tile, wave w = quadrant w; or
  // half a tile, waves (0,1) and (2,3) = the upper / lower 8x4 pixels of its two quadrants; or one list segment --, y = first
  // position of the tile's list, z = how deep the item's pixels reach into it (the forward's work_maxc).  Until round 4 an
  // item's start was a chain of dependent round trips: work list -> ranges, final_T, n_contrib -> maximum over the
  // workgroup (two barriers) -> dL_dpixel, bg -> ids -> records.  Now everything per pixel and the first ids are requested
  // together, right behind the descriptor.
  uint32_t tile = item.x;
  const bool half_item = (tile & BWD_ITEM_HALF) != 0u;
  const uint32_t part = (tile & BWD_ITEM_PART) ? 1u : 0u;
  const bool seg_item = SEG && (tile & BWD_ITEM_SEG) != 0u;  // (SEG: a template switch -- the work list of a view without checkpoints holds no such item)
  const uint32_t seg_first = (tile >> BWD_SEG_SHIFT) & 15u, seg = (tile >> BWD_NSEG_SHIFT) & 15u;  // the run's first / last stride
  tile &= BWD_ITEM_TILE;
  const uint32_t list_base = item.y, tile_max = item.z;
  if (tile_max == 0) return 0u;  // (uniform: nothing of the item's pixels ever contributed)
  // the list positions this item walks: all of [0, tile_max), or a run of strides of them (the stride of the last slot
  // reaches to the end of the list, and so does whatever stride holds the tile's deepest contributor)
  const uint32_t seg_lo = seg_item ? a.ck_pos.pos(seg_first) : 0u;
  const uint32_t nslots = (uint32_t)a.ck_slots;  // slots in use per tile (<= CK_MAX), the stride of the pool and of ck_work
  const uint32_t seg_hi = (seg_item && seg != nslots - 1u) ? min(tile_max, a.ck_pos.pos(seg + 1u)) : tile_max;
  if (seg_lo >= seg_hi) return 0u;  // (uniform)
  PixelWave pw;
  const bool has_pixels = setup_wave(a, tile, half_item ? 2u * part + (uint32_t)(w >> 1) : (uint32_t)w, pw);
  const float pfx = (float)pw.px, pfy = (float)pw.py;
  const float qx0 = (float)(pw.px - (lane & 7)), qy0 = (float)(pw.py - (lane >> 3));  // origin of the wave's 8x8 lane grid
  if (half_item) pw.inside = pw.inside && ((lane >> 5) == (w & 1));  // (lanes of the other half never become live)
  const size_t HW = (size_t)a.H * a.W;
  const bool live = has_pixels && pw.inside;
  // per-pixel inputs: UNCONDITIONAL loads (a lane without a pixel reads pixel 0 and drops the values below; a predicated
  // load makes hipcc wait for the data at the issue point), in front of the walker's first ids
  const size_t pix = live ? (size_t)pw.py * a.W + pw.px : (size_t)0;
  const float T_final_ld = a.final_T[pix];
  const uint32_t n_contrib_ld = a.n_contrib[pix];
  const float dpx_ld[3] = {a.dL_dpix[pix], a.dL_dpix[HW + pix], a.dL_dpix[2 * HW + pix]};
  const float dpd_ld = DEPTH ? a.dL_ddepth[pix] : 0.f;
  const float dpa_ld = ALPHA ? a.dL_dalpha[pix] : 0.f;
  // back to front over the item's positions [seg_lo, seg_hi) of the tile's list, all four waves in the same chunks
  ChunkWalker<false> walk(a, list_base + seg_lo, seg_hi - seg_lo);

  const float T_final = live ? T_final_ld : 0.f;
  float T = T_final;
  const uint32_t last_contributor = live ? n_contrib_ld : 0u;
  const uint32_t maxc = wave_max_u32_dpp(last_contributor);  // (this wave's pixels; the item's is tile_max)
  const float dpx[3] = {live ? dpx_ld[0] : 0.f, live ? dpx_ld[1] : 0.f, live ? dpx_ld[2] : 0.f};
  const float dpd = live ? dpd_ld : 0.f;  // (DEPTH) dL_dout_depth of the pixel
  const float dpa = live ? dpa_ld : 0.f;  // (ALPHA) dL_dout_alpha of the pixel
  const float bg_dot_dpixel = ALPHA ? ((0.f + bg0 * dpx[0]) + bg1 * dpx[1] + bg2 * dpx[2]) - dpa
                                    : (0.f + bg0 * dpx[0]) + bg1 * dpx[1] + bg2 * dpx[2];
  const float neg_Tfinal_bg = -T_final * bg_dot_dpixel;  // the background's share of dL/dalpha is this times 1 / (1 - alpha)
  const float ddelx_dx = 0.5f * a.W, ddely_dy = 0.5f * a.H;

  float B_acc = 0.f, last_cdot = 0.f;  // sum_ch accum_rec[ch]*dL_dpixel[ch], sum_ch last_color[ch]*dL_dpixel[ch]
  float last_alpha = 0.f;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  if (seg_item && last_contributor > seg_hi) {
    // This pixel still contributes BEHIND the segment: it enters at position seg_hi - 1 with the state the sequential walk
    // would have there.  T in front of position seg_hi is the forward's checkpoint; the colour recurrence (accum_rec,
    // backward.cu:515) at that point is the colour of everything behind, over that transmittance:
    //   accum_rec = (C_final - C(seg_hi)) / T(seg_hi),  with nothing pending (last_alpha = 0).
    // Round 5: the colour behind is the SUM of the later segments' own colours (the forward accumulates every segment from
    // zero: slot k + 1 holds segment k's, slot 0 that of segment CK_MAX - 1 and everything after it), smallest first -- as
    // C_final - C(seg_hi) it was a difference of two numbers near 1 divided by a small transmittance.
    const uint32_t pidx = (uint32_t)((pw.py & (TILE - 1)) * TILE + (pw.px & (TILE - 1)));
    const size_t slot0 = (size_t)a.ck_table[tile] * nslots;  // (slot k >= 1: T in front of position pos(k) + segment k - 1's colour)
    uint32_t m = 0u;  // the segment of the pixel's last contributor: the checkpoints at or in front of its position
#pragma unroll
    for (uint32_t k = 1u; k < (uint32_t)CK_MAX; ++k) m += (k < nslots && last_contributor - 1u >= a.ck_pos.pos(k)) ? 1u : 0u;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    // (wave-uniform bounds; a lane takes part from its own m down.  The two slot counts the library itself chooses get a
    //  loop with a constant upper end -- unrolled, as when CK_MAX was the only count: with both ends variable every
    //  iteration waits for its own load, 3-4 % of the whole kernel on the deep-tile views)
    auto add_slot = [&](uint32_t k, uint32_t top) __attribute__((always_inline)) {
      if (k > seg && k <= m) {
        const float4 sk = a.ck_pool[(slot0 + (k + 1u < top ? k + 1u : 0u)) * (TILE * TILE) + pidx];
        b0 += sk.y;
        b1 += sk.z;
        b2 += sk.w;
      }
    };
    auto sum_behind = [&](auto slots_c) __attribute__((always_inline)) {
      constexpr uint32_t S = decltype(slots_c)::value;
#pragma unroll
      for (uint32_t i = 1u; i < S; ++i) add_slot(S - i, S);  // k = S - 1 down to 1
    };
    if (nslots == (uint32_t)CK_MAX / 2u) sum_behind(std::integral_constant<uint32_t, (uint32_t)CK_MAX / 2u>{});
    else if (nslots == (uint32_t)CK_MAX) sum_behind(std::integral_constant<uint32_t, (uint32_t)CK_MAX>{});
    else
      for (uint32_t k = nslots - 1u; k > seg; --k) add_slot(k, nslots);  // (GSR_CK_SLOTS: any other count)
    T = a.ck_pool[(slot0 + seg + 1u) * (TILE * TILE) + pidx].x;
    B_acc = (b0 * dpx[0] + b1 * dpx[1] + b2 * dpx[2]) / T;
  }

  // Flush of one chunk's accumulators (round 6: ONE memory-side request per (tile, instance) instead of up to nine).
  // Device-scope float atomics execute at the memory side on this chip, and what they cost is the REQUEST: a wave instruction's
  // lanes that hit the same 64-byte line travel as one (tools/microbench/atomic_merge.hip: 9 values into each of 4 M random
  // rows -- 1 819 us from four arrays, 37.7 M requests; 206 us into 64-byte rows, 4.2 M requests).  With the nine accumulators
  // of a Gaussian in four arrays every atomic was a request of its own: 47 of K7's 215 us on the headline view, 200 of
  // 757 us on synth-v2 (profiles/r06_c_accumulator_rows.md).  Now a Gaussian's accumulators are ONE 64-byte row of `acc` (ACC_* columns,
  // include/gsr.h), and the flush puts the sixteen columns of a row on sixteen adjacent lanes: instruction j of wave w
  // covers the chunk slots 16 w + 4 j .. + 3.  Lane (slot, column) forms its column's term from the slot's raw moments and
  // the entry's conic / opacity (sco) -- backward.cu:545-554 --, skips what is exactly zero, and the lanes of the raw
  // moments' indices put the LDS accumulator back to zero for the buffer's next chunk.
  auto flush = [&](uint32_t fb, uint32_t fsize) __attribute__((always_inline)) {
    const uint32_t col = (uint32_t)lane & 15u, sub = (uint32_t)lane >> 4;
    // raw moments a column reads: dL_dmean2D needs (1, 2); conic x / y / w: 3 / 4 / 5; opacity: 0; colour: 6 / 7 / 8;
    // (DEPTH) depth: 9; (ABS) the absolute screen-space sums: IABS, IABS + 1
    const uint32_t ia = col == ACC_MEAN2D || col == ACC_MEAN2D + 1u ? 1u
                        : col == ACC_OPACITY ? 0u
                        : col == ACC_CONIC ? 3u : col == ACC_CONIC + 1u ? 4u : col == ACC_CONIC + 3u ? 5u
                        : col >= ACC_COLOR && col < ACC_COLOR + 3u ? 6u + (col - ACC_COLOR)
                        : DEPTH && col == ACC_DEPTH ? 9u
                        : ABS && (col == ACC_ABS2D || col == ACC_ABS2D + 1u) ? (uint32_t)IABS + (col - ACC_ABS2D)
                        : (uint32_t)NM;  // NM: the column is not used
    // ONE exec region around the arithmetic of a flush instruction: the atomic's (the row mask's store and the zeroing are
    // masked stores behind it).  A lane's role follows from its column alone -- which moments it reads, which of the entry's
    // constants it multiplies by --, so the LDS reads are unconditional (a column without a moment reads moment 0 and adds
    // nothing; a column with one moment reads it twice), the candidate terms are each the expression the column's own
    // branch used to hold, operation for operation, and selects choose: a compare -> exec -> VALU turn costs about three
    // selects (tools/microbench/issue_rate.hip), and the dispatch on the column was a chain of up to nine exec regions per
    // instruction (profiles/k7_flush_used_slots_ab.md: 224 -> 122 s_*_saveexec in blend_backward_kernel<0,0,0,0,0>).
    // No 0 * x stands in for "not this column": a non-finite constant of the entry reaches no column that did not multiply
    // by it before.
    const bool has = ia < (uint32_t)NM, mean = ia == 1u, xcol = col == ACC_MEAN2D;
    const bool absc = ABS && has && ia >= (uint32_t)IABS, conic = ia >= 3u && ia <= 5u;
    const uint32_t ra = has ? ia : 0u, rb = mean ? 2u : ra;
    const float scale = (xcol || (ABS && col == ACC_ABS2D)) ? ddelx_dx : ddely_dy;
    const uint32_t w16 = (uint32_t)__builtin_amdgcn_readfirstlane(16 * w);  // (scalar: the loop's exit is a scalar branch)
#pragma unroll
    for (uint32_t jj = 0; jj < 4u; ++jj) {
      const uint32_t p = w16 + 4u * jj + sub;
      if (w16 + 4u * jj >= fsize) break;  // (wave-uniform: slots >= fsize are never added to)
      float* const row = sacc[fb][p];  // (p < 64: a slot >= fsize of the last, partial chunk holds zeros and a stale entry)
      const float ma = row[ra], mb = row[rb];
      const float4 co = sco[fb][p];  // conic.x, conic.y, conic.z, opacity
      const uint32_t id = sid[fb][p];
      // backward.cu:545-546: dL_dmean2D = -o (A t1 + B t2, B t1 + C t2) * (0.5 W, 0.5 H)
      const float c1 = xcol ? co.x : co.y, c2 = xcol ? co.y : co.z;
      float v_mean = -(scale * co.w) * (c1 * ma + c2 * mb);
      // the per-pixel terms of dL_dmean2D in absolute value: |o| 0.5 W sum |A qx + B qy|, |o| 0.5 H sum |B qx + C qy|
      float v_abs = (scale * __builtin_fabsf(co.w)) * ma;
      // backward.cu:549-551: -0.5 o t; opacity (:554), colour (:523), depth: the moment itself
      float v_conic = (-0.5f * co.w) * ma;
      // (keeps the candidates in front of the selects: left alone, hipcc sinks each into a branch on its column again)
      if constexpr (ABS) asm volatile("" : "+v"(v_mean), "+v"(v_abs), "+v"(v_conic));
      else asm volatile("" : "+v"(v_mean), "+v"(v_conic));
      const float val = mean ? v_mean : absc ? v_abs : conic ? v_conic : ma;
      const bool add = has && p < fsize && (ma != 0.f || mb != 0.f);  // (exact zeros are skipped)
      if (add) unsafeAtomicAdd(&a.acc[(size_t)id * ACC_ROW + col], val);
      if (a.touched != nullptr) {  // (wave-uniform) the exchange's row mask, without a pass over the table: lane 15 of a
        const uint64_t nzm = __ballot(add);  // group marks the group's Gaussian if any of its columns was added to
        if (col == 15u && ((nzm >> (16u * sub)) & 0xffffull) != 0ull) a.touched[id] = 1;
      }
      // (every read of this instruction precedes it: one wave, program order.  The rows >= fsize are zero already: the
      // store's mask is the column's alone.  And the store races with no ds_add_f32: fb is the idle parity -- this
      // iteration's groups add to the other buffer, and the next adds to fb lie behind barrier (B))
      if (col < (uint32_t)NM) row[col] = 0.f;
    }
  };

  // The flush of chunk k is DEFERRED into iteration k + 1 (round 5), behind the walker's prefetch loads: a wave's vector
  // memory operations retire in order, so the wait for the next chunk's records at the top of an iteration also waited for
  // the memory-side float atomics the flush had issued a few instructions earlier (ISA: s_waitcnt vmcnt(0) in the loop
  // header) -- one atomic round trip per chunk on every wave's critical path.  Now the atomics of chunk k have the whole
  // group loop of chunk k + 1 to complete.  The accumulators, sid and sco are double-buffered by chunk parity, which also
  // removes one of the two workgroup barriers per chunk: chunk k + 1 writes buffer (k + 1) & 1, whose last flush (chunk
  // k - 1) ran in iteration k, in front of barrier (B) of that iteration.
  uint32_t pend_size = 0u;  // slots of the previous chunk still to be flushed (0: none)
  for (; walk.valid(); walk.advance()) {
    const uint32_t csize = walk.chunk_size();
    const uint32_t cb = walk.chunk & 1u;
    if (w == 0 && (uint32_t)lane < csize) {
      sid[cb][lane] = walk.cur.id;
      sco[cb][lane] = walk.cur.r0;
    }
    const uint32_t pos = seg_lo + walk.lane_pos();
    // pixels that can still use an entry of this chunk: their last contributor lies above the chunk's lowest position;
    // the cull rectangle is their bounding box (the first chunks of a long list are walked for a few stragglers only)
    const uint32_t chunk_lo = seg_hi - min(seg_hi - seg_lo, (walk.chunk + 1u) * (uint32_t)WAVE);
    const uint64_t live_m = __ballot(last_contributor > chunk_lo);
    bool keep = false;
    if (live_m != 0) keep = chunk_cull(live_m, qx0, qy0, ((uint32_t)lane < csize) && (pos < maxc), walk.cur);
    const uint64_t m = __ballot(keep);
    const uint32_t cnt = (uint32_t)__popcll(m);
    const uint32_t cnt4 = (cnt + GROUP - 1) & ~(uint32_t)(GROUP - 1);
    if (keep) {
      const uint32_t slot = (uint32_t)__popcll(m & lt_mask);
      // conic pre-scaled as in the forward: (-0.5 A, -B, -0.5 C), exact
      s0[w][slot] = make_float4(-0.5f * walk.cur.r0.x, -walk.cur.r0.y, -0.5f * walk.cur.r0.z, walk.cur.r0.w);
      s1[w][slot] = make_float4(walk.cur.r1.x, walk.cur.r1.y, walk.cur.r1.z, __uint_as_float(pos));
      // .w carries the entry's index inside the chunk (= the lane that holds it): the LDS accumulator slot
      s2[w][slot] = make_float4(walk.cur.r2.x, walk.cur.r2.y, walk.cur.r2.z, __uint_as_float((uint32_t)lane));
    }
    if ((uint32_t)lane >= cnt && (uint32_t)lane < cnt4) {
      s0[w][lane] = make_float4(0.f, 0.f, 0.f, 0.f);  // null entry: alpha 0 => never contributes
      s1[w][lane] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xffffffffu));
      s2[w][lane] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0u));
    }
    wave_lds_sync();
    if (pend_size != 0u) flush(cb ^ 1u, pend_size);  // (behind barrier (B) of the previous iteration)
    pend_size = csize;

    for (uint32_t j = 0; j < cnt4; j += GROUP) {
      float G[GROUP], al[GROUP], dxs[GROUP], dys[GROUP];
      bool contrib[GROUP];
      float4 cos_[GROUP], cols[GROUP];
      float dep[GROUP];  // (DEPTH) the entries' view-space depths
      bool any = false;
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        const float4 g = s1[w][j + u];
        dep[u] = DEPTH ? g.z : 0.f;
        cos_[u] = s0[w][j + u];
        cols[u] = s2[w][j + u];
        const uint32_t c = __float_as_uint(g.w);  // 0-based position of this instance in the tile list
        dxs[u] = g.x - pfx;
        dys[u] = g.y - pfy;
        const float power = blend_power_prescaled(cos_[u].x, cos_[u].y, cos_[u].z, dxs[u], dys[u]);
        G[u] = blend_exp<FAST>(power);  // only used where alpha >= 1/255, i.e. far above the clamp
        al[u] = fminf(0.99f, cos_[u].w * G[u]);
        contrib[u] = (c < last_contributor) && !(power > 0.0f) && !(al[u] < 1.0f / 255.0f);
        any = any || contrib[u];
      }
      if (!__any(any)) continue;  // wave-uniform

      float v[NM][GROUP];
      {
#pragma clang fp contract(fast)  // gradients are tolerance-checked (<= 1e-5), not bit-compared: let a*b+c fuse here
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
          // (accum_rec_step: a lane that does not contribute keeps its state through selects and hands zeros on)
          const bool on = contrib[u];
          const float alpha = on ? al[u] : 0.f;
          const float inv_one_m = rcp_refined(1.f - alpha);
          // (DEPTH: the depth channel joins the collapsed recurrence, d * dL_dD; its background is 0)
          const float cdot = DEPTH ? cols[u].x * dpx[0] + cols[u].y * dpx[1] + cols[u].z * dpx[2] + dep[u] * dpd
                                   : cols[u].x * dpx[0] + cols[u].y * dpx[1] + cols[u].z * dpx[2];
          const RecStep rs = accum_rec_step(T, B_acc, last_alpha, last_cdot, inv_one_m, cdot);
          T = rs.T;
          B_acc = rs.B_acc;
          const float dL_dalpha = rs.dL_dalpha + neg_Tfinal_bg * inv_one_m;
          last_alpha = alpha;
          last_cdot = on ? cdot : last_cdot;
          const float q = on ? G[u] * dL_dalpha : 0.f;
          const float mD = alpha * T;  // dchannel_dcolor (0 for a skipped lane)
          geometry_moments(v, u, q, dxs[u], dys[u]);
          v[6][u] = mD * dpx[0];
          v[7][u] = mD * dpx[1];
          v[8][u] = mD * dpx[2];
          if constexpr (DEPTH) v[9][u] = mD * dpd;  // dL/dd of the entry
          if constexpr (ABS) {  // |A qx + B qy|, |B qx + C qy| (cos_ = (-0.5 A, -B, -0.5 C): both signs flipped, exact scaling)
            const float qx = v[1][u], qy = v[2][u];  // (moments 1, 2: q dx, q dy)
            v[IABS][u] = __builtin_fabsf(2.f * cos_[u].x * qx + cos_[u].y * qy);
            v[IABS + 1][u] = __builtin_fabsf(cos_[u].y * qx + 2.f * cos_[u].z * qy);
          }
        }
      }
      // 4-entry packed wave reduction: afterwards a lane holds the wave total of moment tail_term of entry j + tail_entry,
      // and ONE ds_add_f32 (the lowest lane of every total, 4 NM lanes) adds the RAW moments to the tile-level
      // accumulator of the entry's chunk slot (they are relative to the entry's own mean, so the quadrants' sums simply
      // add; the flush turns them into the reference's terms).  A null entry adds zeros to slot 0.
      // (masked row stages except with ABS: those kernels sit at 128 VGPRs and the ten-pair statements make them spill)
      float tot = wave_sum4_pack<NM, !ABS>(v);
      // (keeps the reduction whole in front of the masked tail)
      asm volatile("" : "+v"(tot));
      if (tail_adds) {
        const uint32_t my_slot = __float_as_uint(s2[w][j + tail_entry].w);
        atomicAdd(&sacc[cb][my_slot][tail_term], tot);
      }
    }
    __syncthreads();  // (B) every quadrant's contribution to this chunk is in sacc[cb]
  }
  // the last chunk (the next item's first LDS write lies behind barriers).  The walker's last prefetch -- chunks beyond the
  // end, never used -- is drained first: the flush re-uses its registers, and behind the first atomic every such wait
  // would be one for the atomic.
  asm volatile("" ::"v"(walk.nxt.r0.x), "v"(walk.nxt.r1.x), "v"(walk.nxt.r2.x), "v"(walk.id_next), "v"(walk.id_next2));
  if (pend_size != 0u) flush((walk.chunk - 1u) & 1u, pend_size);
  return seg_hi - seg_lo;
}

template <bool FAST, bool SEG, bool DEPTH, bool ABS, bool ALPHA>
__global__ void __launch_bounds__(WAVE* BWD_WAVES) __attribute__((amdgpu_waves_per_eu(4, 4)))
blend_backward_kernel(const BlendArgs a) {
  constexpr int LDS_ROW = bwd_lds_row<DEPTH, ABS>();
  __shared__ float4 s0[BWD_WAVES][WAVE], s1[BWD_WAVES][WAVE], s2[BWD_WAVES][WAVE];
  __shared__ uint32_t sid[2][WAVE];  // (sid, sco, sacc: double-buffered by chunk parity, see backward_tile)
  __shared__ float4 sco[2][WAVE];
  __shared__ float sacc[2][WAVE][LDS_ROW];  // raw moments 0..8 (DEPTH: 0..9; ABS: two more) of every chunk slot (row stride 9 / 11 / 13: odd, the four rows of a flush instruction spread over the banks)
  __shared__ uint32_t s_item;
  for (int i = threadIdx.x; i < 2 * WAVE * LDS_ROW; i += WAVE * BWD_WAVES) (&sacc[0][0][0])[i] = 0.f;
  // (element i was zeroed by thread i % 256, i.e. by any wave: with the deferred flush the placement-assigned first item
  // reaches its first ds_add_f32 without passing a workgroup barrier otherwise.  Once per kernel, not per item.)
  __syncthreads();
  const float bg0 = wave_uniform(a.bg[0]), bg1 = wave_uniform(a.bg[1]), bg2 = wave_uniform(a.bg[2]);
  // item-granular queue: queue x (one per XCD) owns items x, x+8, ... of the backward's work list
  const uint32_t x = xcc_id() & 7u;
  const uint32_t nwork = a.bwd_meta[0];
  const uint32_t n_x = nwork > x ? (nwork - x + 7u) / 8u : 0u;
  uint32_t* head = a.queue + x * QUEUE_STRIDE;
  // debug timing (gsr_debug_blend_backward_profile): per workgroup start / end, tiles, longest and first tile
  const bool prof = a.profile != nullptr;
  uint64_t t_begin = 0, t_tile = 0, longest = 0, first = 0;
  uint32_t ntiles = 0, west = 0;
  if (prof) t_begin = __builtin_amdgcn_s_memtime();
  auto run_tile = [&](uint32_t index) {
    if (prof) t_tile = __builtin_amdgcn_s_memtime();
    const uint4 item = load_backward_item(a, index);
    const uint32_t tile = item.x;
    const uint32_t tmax = backward_tile<FAST, SEG, DEPTH, ABS, ALPHA>(a, item, bg0, bg1, bg2, s0, s1, s2, sid, sco, sacc);
    if (prof) {
      const uint64_t d = __builtin_amdgcn_s_memtime() - t_tile;
      if (a.profile_items != nullptr && threadIdx.x == 0 && a.work_est != nullptr) {
        // per item: cycles, the forward's per-quadrant counts of the tile, positions walked, item code
        const uint32_t tt = tile & BWD_ITEM_TILE;
        uint64_t* r = a.profile_items + ((size_t)tt * 2 + ((tile & BWD_ITEM_PART) ? 1 : 0)) * 4;
        const uint4 e = reinterpret_cast<const uint4*>(a.work_est)[tt];
        r[0] = d;
        r[1] = ((uint64_t)e.x) | ((uint64_t)e.y << 16) | ((uint64_t)e.z << 32) | ((uint64_t)e.w << 48);
        r[2] = tmax;
        r[3] = tile;
      }
      if (ntiles == 0) first = d;
      longest = d > longest ? d : longest;
      ntiles++;
      if (a.work_est != nullptr) {
        const uint32_t tt = tile & BWD_ITEM_TILE;
        if (tile & BWD_ITEM_HALF) {
          const uint32_t q0 = (tile & BWD_ITEM_PART) ? 2u : 0u;
          west += a.work_est[4u * tt + q0] + a.work_est[4u * tt + q0 + 1];
        } else {
          west += a.work_est[4u * tt] + a.work_est[4u * tt + 1] + a.work_est[4u * tt + 2] + a.work_est[4u * tt + 3];
        }
      }
    }
  };
  // first item assigned by placement (see first_item_of_block), the rest popped
  uint32_t x0, base;
  const uint32_t q0 = first_item_of_block((uint32_t)a.units, x0, base);
  {
    const uint32_t n0 = nwork > x0 ? (nwork - x0 + 7u) / 8u : 0u;
    if (q0 < n0) run_tile(x0 + 8u * q0);
  }
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_item = base + __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t q = s_item;
    if (q >= n_x) break;
    run_tile(x + 8u * q);
  }
  if (prof && threadIdx.x == 0) {
    uint64_t* rec = a.profile + (size_t)blockIdx.x * 8;
    rec[0] = t_begin;
    rec[1] = __builtin_amdgcn_s_memtime();
    rec[2] = ((uint64_t)xcc_id() << 32) | (uint64_t)__builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4);  // | HW_REG_HW_ID
    rec[3] = ((uint64_t)ntiles << 32) | (uint64_t)west;
    rec[4] = longest;
    rec[5] = first;
  }
  if (a.self_reset && threadIdx.x == 0) retire_queue(a.queue);
}

// ----------------------------------------------------------------------------------
// K12: renderCUDA_apply_weights, DGR/cuda_rasterizer/apply_weights.cu:239-356.
// Same traversal / termination as K6; every blended (pixel, instance) adds the pixel's
// mask value(s) to weights[id] and C to cnt[id] (the reference increments cnt inside its
// channel loop, apply_weights.cu:331-339).
// ----------------------------------------------------------------------------------
// The traversal is walk_front_to_back (K6's inner loop since round 6).  The payload: what a pixel adds for the four entries
// of a group (its mask value per channel, and 1 for the count) is summed over the wave four values at a time
// (wave_sum4_to_rows: 10 instructions instead of 4 x 8), and a chunk's totals leave with one atomic per (entry, channel).
template <int C, int SPLIT, bool FAST>
__device__ __forceinline__ void trace_item(const BlendArgs& a, uint32_t tile, uint32_t quad) {
  PixelWave pw;
  ItemBox box;
  if (!setup_item<SPLIT>(a, tile, quad, pw, box)) return;
  const int lane = lane_id();
  const uint2 range = a.ranges[pw.tile];
  if (range.y <= range.x) return;
  (void)box;  // (the cull rectangle follows the pixels that are still live, live_pixel_box)
  const size_t pix = (size_t)pw.py * a.W + pw.px, HW = (size_t)a.H * a.W;
  float Cw[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) Cw[ch] = pw.inside ? a.image_weights[(size_t)ch * HW + pix] : 0.f;
  __shared__ uint32_t sid[WAVE];
  __shared__ float sacc[C][WAVE];
  __shared__ float scnt[WAVE];
  const bool row_end = (lane & 15) == 15;
  walk_front_to_back<FAST>(
      a, pw, range, [&](uint32_t slot, const Entry& e) __attribute__((always_inline)) { sid[slot] = e.id; },
      [&](uint32_t j, const bool(&hit)[GROUP], const float(&)[GROUP]) __attribute__((always_inline)) {
        const uint32_t e = j + ((uint32_t)lane >> 4);  // the entry whose totals end up in this lane's row
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          const float z = wave_sum4_to_rows(hit[0] ? Cw[ch] : 0.f, hit[1] ? Cw[ch] : 0.f, hit[2] ? Cw[ch] : 0.f, hit[3] ? Cw[ch] : 0.f);
          if (row_end) sacc[ch][e] = z;
        }
        const float zc = wave_sum4_to_rows(hit[0] ? 1.0f : 0.0f, hit[1] ? 1.0f : 0.0f, hit[2] ? 1.0f : 0.0f, hit[3] ? 1.0f : 0.0f);
        if (row_end) scnt[e] = zc;
      },
      [&](uint32_t evaluated) __attribute__((always_inline)) {
        __syncthreads();
        // (the groups behind a break wrote nothing: their slots hold an earlier chunk's values)
        if ((uint32_t)lane < evaluated) {
          const int cn = (int)scnt[lane] * C;
          if (cn != 0) {
            const size_t id = sid[lane];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) unsafeAtomicAdd(&a.weights[id * C + ch], sacc[ch][lane]);
            atomicAdd(&a.cnt[id], cn);
          }
        }
      });
}
template <int C, int SPLIT, bool FAST>
__global__ void __launch_bounds__(WAVE) trace_weights_kernel(const BlendArgs a) {
  run_work_queue<SPLIT>(a, false, [&](uint32_t tile, uint32_t quad, bool) __attribute__((always_inline)) { trace_item<C, SPLIT, FAST>(a, tile, quad); });
}

// ----------------------------------------------------------------------------------
// Contribution statistics and the pick buffer (gsr_trace_contributions): K12's sibling that KEEPS the blending weight
// w = alpha T of every (pixel, entry) the walk hands out.  No reference counterpart.  Per Gaussian g, in the int64 row
// stats[g] (3 + C columns, accumulated in place):
//   [0]     sum over the pixels that blend g of q(w),  q(x) = (uint32) trunc(x 2^32)   (w <= 0.99: q fits 32 bits)
//   [1]     pixels whose largest weight is g's (the pick buffer's histogram)
//   [2]     the largest w, as the float's bit pattern (w > 0: the unsigned order of the patterns is the floats')
//   [3 + c] sum of q(w * m_c), m_c = the pixel's mask value of channel c clamped to [0, 1] (NaN -> 0), one binary32 multiply
// Every accumulation is an integer add or an integer max, so a table does not depend on the grid, the quadrant cut, the
// arrival order or the order of the views.  The wave sums stay on the float reduction K12 uses (wave_sum4_to_rows): q is
// summed as its two 16-bit halves, each total <= 64 x 65535 < 2^24 and therefore exact in binary32 in any order, and
// put together again as 64 bits behind the chunk.  A chunk's survivors leave with at most one atomic per column.
// The per-pixel largest weight and its Gaussian live in registers across the chunks (strictly greater replaces: among
// equal weights the front-most entry of the list wins); column 1 gets one add per pixel at the end of the item.
// What is new beside a view's BlendArgs travels as a second kernel argument, as FeatureArgs does.
// ----------------------------------------------------------------------------------
struct ContribArgs {
  unsigned long long* stats;  // (P, 3 + C), the int64 table (its values are never negative)
  int32_t* top_id;            // (H,W) | null: fully written, -1 where the pixel blends nothing
  float* top_weight;          // (H,W) | null: fully written, 0 where the pixel blends nothing
};
// max of each of four per-lane values over the 64 lanes: wave_fold4_to_rows / wave_sum4_to_rows with an unsigned max (its
// identity is the 0 a DPP lane without a source reads).  The maximum of value r ends up in lane 16 r + 15.
__device__ __forceinline__ uint32_t wave_max4_to_rows(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  {
    auto r = __builtin_amdgcn_permlane32_swap(a, c, false, false);
    a = r[0];
    c = r[1];
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(b, d, false, false);
    b = r[0];
    d = r[1];
  }
  uint32_t x = max(a, c), y = max(b, d);  // lanes 0-31: a | b, 32-63: c | d
  {
    auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    x = r[0];
    y = r[1];
  }
  uint32_t z = max(x, y);  // rows: a, b, c, d
  z = max(z, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)z, 0x111, 0xf, 0xf, false));
  z = max(z, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)z, 0x112, 0xf, 0xf, false));
  z = max(z, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)z, 0x114, 0xf, 0xf, false));
  z = max(z, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)z, 0x118, 0xf, 0xf, false));
  return z;
}
template <int C, int SPLIT, bool FAST>
__device__ __forceinline__ void contrib_item(const BlendArgs& a, const ContribArgs& f, uint32_t tile, uint32_t quad) {
  PixelWave pw;
  ItemBox box;
  if (!setup_item<SPLIT>(a, tile, quad, pw, box)) return;
  (void)box;
  const int lane = lane_id();
  const uint2 range = a.ranges[pw.tile];
  const size_t pix = (size_t)pw.py * a.W + pw.px, HW = (size_t)a.H * a.W;
  constexpr int COLS = 3 + C, SUMS = 1 + C;  // sums: the total, then the channels
  float m[SUMS];                             // (m[0] unused: the total's "mask" is 1)
  m[0] = 1.0f;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const float v = pw.inside ? a.image_weights[(size_t)ch * HW + pix] : 0.f;
    m[1 + ch] = v > 0.0f ? fminf(v, 1.0f) : 0.0f;  // (NaN > 0 is false)
  }
  __shared__ __align__(16) uint32_t sid[WAVE];
  __shared__ float slo[SUMS][WAVE], shi[SUMS][WAVE];
  __shared__ uint32_t smax[WAVE];
  const bool row_end = (lane & 15) == 15;
  float best_w = 0.0f;
  int32_t best_id = -1;
  walk_front_to_back<FAST>(
      a, pw, range, [&](uint32_t slot, const Entry& e) __attribute__((always_inline)) { sid[slot] = e.id; },
      [&](uint32_t j, const bool(&hit)[GROUP], const float(&w)[GROUP]) __attribute__((always_inline)) {
        const uint32_t e = j + ((uint32_t)lane >> 4);  // the entry whose totals end up in this lane's row
        const uint4 ids = *reinterpret_cast<const uint4*>(&sid[j]);  // (j is a multiple of GROUP; uniform: one broadcast read)
        const uint32_t id4[GROUP] = {ids.x, ids.y, ids.z, ids.w};
        float wh[GROUP];  // the weight where the pixel blends the entry, 0 where it does not (w is meaningless there)
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
          wh[u] = hit[u] ? w[u] : 0.0f;
          const bool better = wh[u] > best_w;
          best_w = better ? wh[u] : best_w;
          best_id = better ? (int32_t)id4[u] : best_id;
        }
#pragma unroll
        for (int k = 0; k < SUMS; ++k) {
          float lo[GROUP], hi[GROUP];
#pragma unroll
          for (int u = 0; u < GROUP; ++u) {
            const uint32_t q = (uint32_t)((k == 0 ? wh[u] : wh[u] * m[k]) * 4294967296.0f);
            lo[u] = (float)(q & 0xffffu);
            hi[u] = (float)(q >> 16);
          }
          const float zl = wave_sum4_to_rows(lo[0], lo[1], lo[2], lo[3]);
          const float zh = wave_sum4_to_rows(hi[0], hi[1], hi[2], hi[3]);
          if (row_end) {
            slo[k][e] = zl;
            shi[k][e] = zh;
          }
        }
        const uint32_t zm = wave_max4_to_rows(__float_as_uint(wh[0]), __float_as_uint(wh[1]), __float_as_uint(wh[2]), __float_as_uint(wh[3]));
        if (row_end) smax[e] = zm;
      },
      [&](uint32_t evaluated) __attribute__((always_inline)) {
        __syncthreads();
        // (the groups behind a break wrote nothing: their slots hold an earlier chunk's values)
        if ((uint32_t)lane < evaluated) {
          const unsigned long long total = ((unsigned long long)(uint32_t)shi[0][lane] << 16) + (uint32_t)slo[0][lane];
          if (total != 0ull) {  // some pixel blends the entry (q(w) > 0 for every blended w: w >= 1e-4 / 255)
            unsigned long long* row = f.stats + (size_t)sid[lane] * COLS;
            atomicAdd(row, total);
            atomicMax(row + 2, (unsigned long long)smax[lane]);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
              const unsigned long long wq = ((unsigned long long)(uint32_t)shi[1 + ch][lane] << 16) + (uint32_t)slo[1 + ch][lane];
              if (wq != 0ull) atomicAdd(row + 3 + ch, wq);
            }
          }
        }
      });
  if (pw.inside) {
    if (f.top_id != nullptr) f.top_id[pix] = best_id;
    if (f.top_weight != nullptr) f.top_weight[pix] = best_w;
    if (best_id >= 0) atomicAdd(f.stats + (size_t)best_id * COLS + 1, 1ull);
  }
}
template <int C, int SPLIT, bool FAST>
__global__ void __launch_bounds__(WAVE) trace_contributions_kernel(const BlendArgs a, const ContribArgs f) {
  // (the tiles no Gaussian touches are items only where a pixel image wants their -1 / 0)
  run_work_queue<SPLIT>(a, f.top_id != nullptr || f.top_weight != nullptr, [&](uint32_t tile, uint32_t quad, bool empty) __attribute__((always_inline)) {
    if (!empty) {
      contrib_item<C, SPLIT, FAST>(a, f, tile, quad);
    } else {
      for_each_pixel_of_tile(a, tile, [&](size_t pix, size_t) __attribute__((always_inline)) {
        if (f.top_id != nullptr) f.top_id[pix] = -1;
        if (f.top_weight != nullptr) f.top_weight[pix] = 0.0f;
      });
    }
  });
}

// ----------------------------------------------------------------------------------
// Feature rendering: per-Gaussian feature vectors of C channels, alpha-composited into a (C,H,W) image on background 0
// (gsr_blend_forward_features), and its backward (gsr_blend_backward_features).  No reference counterpart (the reference
// composites three channels); the N-D `colors` of current 3DGS rasterizers.
// The channels are walked in BLOCKS of FEAT_BLOCK = 16 (one 64-byte line of a feature row): alpha and T of a (pixel, entry)
// pair are evaluated once per block, not once per three channels as a chain of auxiliary renders would.
// What the two kernels need beyond a view's BlendArgs travels as a second kernel argument: BlendArgs, and with it the
// argument layout of every other kernel, keeps its size.
// ----------------------------------------------------------------------------------
constexpr int FEAT_BLOCK = 16;
struct FeatureArgs {
  const float* features;   // (P,C) row-major
  float* out;              // forward: (C,H,W), fully written
  const float* dL_dimage;  // backward: (C,H,W), the gradient of `out`
  float* dL_dfeatures;     // backward: (P,C), added into (the caller zeroes it)
  int C;
};

// One forward item: walk_front_to_back once per channel block, and per blended (pixel, entry) K6's accumulation
// C_c = fma(f_c, alpha T, C_c) for the 16 channels of the block -- channel c of the image equals, as floats, channel c % 3 of an
// auxiliary render of features[:, 3 (c / 3) : + 3].  The accumulation is a lane-masked region, as K6's masked form: a feature of
// an entry the pixel skips is never read into the sum (0 x NaN).
template <bool FAST>
__device__ __forceinline__ void feature_forward_item(const BlendArgs& a, const FeatureArgs& f, uint32_t tile, uint32_t quad) {
  PixelWave pw;
  ItemBox box;
  if (!setup_item<1>(a, tile, quad, pw, box)) return;
  (void)box;
  const uint2 range = a.ranges[pw.tile];
  const size_t pix = (size_t)pw.py * a.W + pw.px, HW = (size_t)a.H * a.W;
  __shared__ __align__(16) float sfeat[WAVE][FEAT_BLOCK];
  const int C = f.C;
  for (int c0 = 0; c0 < C; c0 += FEAT_BLOCK) {
    const int nch = min(FEAT_BLOCK, C - c0);  // (the last block may be partial: its missing channels blend zeros)
    float F[FEAT_BLOCK];
#pragma unroll
    for (int k = 0; k < FEAT_BLOCK; ++k) F[k] = 0.f;
    walk_front_to_back<FAST>(
        a, pw, range,
        [&](uint32_t slot, const Entry& e) __attribute__((always_inline)) {
          const float* __restrict__ fr = f.features + (size_t)e.id * (size_t)C + c0;
#pragma unroll
          for (int k = 0; k < FEAT_BLOCK; ++k) {
            const float v = fr[min(k, nch - 1)];  // (unconditional and in bounds; a channel beyond the last one is zero)
            sfeat[slot][k] = k < nch ? v : 0.f;
          }
        },
        [&](uint32_t j, const bool(&hit)[GROUP], const float(&w)[GROUP]) __attribute__((always_inline)) {
#pragma unroll
          for (int u = 0; u < GROUP; ++u) {
            if (hit[u]) {  // the pixel blends the entry: w = alpha T
              const float4* fp = reinterpret_cast<const float4*>(&sfeat[j + u][0]);
#pragma unroll
              for (int k4 = 0; k4 < FEAT_BLOCK / 4; ++k4) {
                const float4 v = fp[k4];
                F[4 * k4] = __builtin_fmaf(v.x, w[u], F[4 * k4]);
                F[4 * k4 + 1] = __builtin_fmaf(v.y, w[u], F[4 * k4 + 1]);
                F[4 * k4 + 2] = __builtin_fmaf(v.z, w[u], F[4 * k4 + 2]);
                F[4 * k4 + 3] = __builtin_fmaf(v.w, w[u], F[4 * k4 + 3]);
              }
            }
          }
        },
        [](uint32_t) __attribute__((always_inline)) {});
    if (pw.inside) {
#pragma unroll
      for (int k = 0; k < FEAT_BLOCK; ++k)
        if (k < nch) f.out[(size_t)(c0 + k) * HW + pix] = F[k];
    }
  }
}
template <bool FAST>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
feature_forward_kernel(const BlendArgs a, const FeatureArgs f) {
  run_work_queue<1>(a, true, [&](uint32_t tile, uint32_t quad, bool empty) __attribute__((always_inline)) {
    if (!empty) {
      feature_forward_item<FAST>(a, f, tile, quad);
    } else {  // a tile no Gaussian touches: zeros
      for_each_pixel_of_tile(a, tile, [&](size_t pix, size_t HW) __attribute__((always_inline)) {
        for (int c = 0; c < f.C; ++c) f.out[(size_t)c * HW + pix] = 0.f;
      });
    }
  });
}

// The feature backward: K7's workgroup (the four quadrant waves of a tile, or of half a heavy one), walking the first
// n_contrib entries of every pixel back to front from final_T, once per channel block.  It needs NO checkpoints and its
// work list holds NO list segments (the forward's checkpoints hold no features): views with long lists take longer than the
// colour backward, as with gsr_blend_backward_depth.
// Mathematics (background 0): F_c = sum_i f_ic alpha_i T_i.  With rec_c the colour behind entry i (the reference's
// accum_rec recurrence, backward.cu:515),
//   dL/dalpha_i = T_i sum_c (f_ic - rec_c) gF_c,      dL/df_ic = alpha_i T_i gF_c.
// As in K7 the recurrence is linear and gF is constant for the pixel, so B = sum_c rec_c gF_c follows the same recurrence
// with the scalar cdot = sum_c f_ic gF_c: one scalar of state per lane whatever the block's width.
// Per entry a wave reduces the six raw geometry moments of q = G dL/dalpha (K7's moments 0 .. 5: q, q dx, q dy, q dx dx,
// q dx dy, q dy dy) and the 16 feature terms; the four waves add both into one LDS row per chunk slot (22 floats in rows of
// 23: odd), and the flush -- deferred by a chunk, as K7's -- turns a row into TWO memory-side requests: the geometry columns
// ACC_MEAN2D, ACC_OPACITY, ACC_CONIC of the Gaussian's accumulator row in K7's conventions (the share of dL/dalpha is linear
// in it: every channel block adds its own), and the 16 channels of the block on 16 adjacent lanes into dL_dfeatures.
constexpr int FEAT_NM = 6;
// Three workgroups per CU, not K7's four: next to K7's state a lane keeps the 16 pixel gradients of the block, and with
// the 128 registers of four waves per SIMD the compiler spills 45 of them to scratch memory; with 168 it spills none.
constexpr int FEAT_BWD_WAVES_PER_SIMD = 3;
constexpr int FEAT_LDS_ROW = FEAT_NM + FEAT_BLOCK + 1;
constexpr int FEAT_HALF = FEAT_BLOCK / 2;  // channels reduced at once: 8 x 4 entries, every total in two lanes
static_assert(pack_lanes<FEAT_NM>().ok && pack_lanes<FEAT_HALF>().ok, "every moment / channel of every entry reaches a lane");
// wave_sum4_pack<NK> of the outer product v[k][u] = m[u] g[k] without forming its 4 NK registers: the first stage pairs the
// entries (u, u + 1) of one channel, so its selects move onto m (four for the whole product) and its output is two
// products and a DPP add.  The lane that ends up with a value is pack_lanes<NK>()'s.
template <int NK>
__device__ __forceinline__ float wave_sum4_pack_outer(const float (&m)[GROUP], const float* g) {
  const int lane = lane_id();
  constexpr int N1 = NK * GROUP / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2, N5 = (N4 + 1) / 2;
  static_assert((N5 + 1) / 2 == 1, "six halvings leave one register");
  const bool second = (lane & 8) != 0;
  const float keep0 = second ? m[1] : m[0], give0 = second ? m[0] : m[1];
  const float keep1 = second ? m[3] : m[2], give1 = second ? m[2] : m[3];
  auto other = [](float x) __attribute__((always_inline)) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), PackStage<8>::ctrl, 0xf, 0xf, true));
  };
  float z[N1];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    z[2 * k] = keep0 * g[k] + other(give0 * g[k]);
    z[2 * k + 1] = keep1 * g[k] + other(give1 * g[k]);
  }
  pack_stage<4, N1>(z, lane);
  pack_stage<2, N2>(z, lane);
  pack_stage<1, N3>(z, lane);
  pack_stage<32, N4>(z, lane);
  pack_stage<16, N5>(z, lane);
  return z[0];
}

template <bool FAST>
__device__ __forceinline__ void feature_backward_tile(const BlendArgs& a, const FeatureArgs& f, const uint4 item,
                                                      float4 (*s0)[WAVE], float4 (*s1)[WAVE], float (*sfeat)[WAVE][FEAT_BLOCK],
                                                      uint32_t (*sid)[WAVE], float4 (*sco)[WAVE],
                                                      float (*sacc)[WAVE][FEAT_LDS_ROW]) {
  const int w = (int)(threadIdx.x >> 6), lane = lane_id();
  constexpr PackLanes tg = pack_lanes<FEAT_NM>(), tf = pack_lanes<FEAT_HALF>();
  auto bit = [lane](uint64_t plane) __attribute__((always_inline)) { return (uint32_t)(plane >> (uint32_t)lane) & 1u; };
  const uint32_t g_term = bit(tg.term_bit[0]) | bit(tg.term_bit[1]) << 1 | bit(tg.term_bit[2]) << 2 | bit(tg.term_bit[3]) << 3;
  const uint32_t g_entry = bit(tg.entry_bit[0]) | bit(tg.entry_bit[1]) << 1;
  const bool g_adds = bit(tg.adds) != 0u;
  const uint32_t f_term = bit(tf.term_bit[0]) | bit(tf.term_bit[1]) << 1 | bit(tf.term_bit[2]) << 2 | bit(tf.term_bit[3]) << 3;
  const uint32_t f_entry = bit(tf.entry_bit[0]) | bit(tf.entry_bit[1]) << 1;
  const bool f_adds = bit(tf.adds) != 0u;
  // the item: a whole tile (wave w = quadrant w) or half of one (K7's item codes; the work list is built without segments)
  uint32_t tile = item.x;
  const bool half_item = (tile & BWD_ITEM_HALF) != 0u;
  const uint32_t part = (tile & BWD_ITEM_PART) ? 1u : 0u;
  tile &= BWD_ITEM_TILE;
  const uint32_t list_base = item.y, tile_max = item.z;
  if (tile_max == 0) return;  // (uniform: nothing of the item's pixels ever contributed)
  PixelWave pw;
  const bool has_pixels = setup_wave(a, tile, half_item ? 2u * part + (uint32_t)(w >> 1) : (uint32_t)w, pw);
  const float pfx = (float)pw.px, pfy = (float)pw.py;
  const float qx0 = (float)(pw.px - (lane & 7)), qy0 = (float)(pw.py - (lane >> 3));
  if (half_item) pw.inside = pw.inside && ((lane >> 5) == (w & 1));
  const size_t HW = (size_t)a.H * a.W;
  const bool live = has_pixels && pw.inside;
  const size_t pix = live ? (size_t)pw.py * a.W + pw.px : (size_t)0;
  const float T_final_ld = a.final_T[pix];
  const uint32_t n_contrib_ld = a.n_contrib[pix];
  const float T_final = live ? T_final_ld : 0.f;
  const uint32_t last_contributor = live ? n_contrib_ld : 0u;
  const uint32_t maxc = wave_max_u32_dpp(last_contributor);
  const float ddelx_dx = 0.5f * a.W, ddely_dy = 0.5f * a.H;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  const int C = f.C;
  // the features of a chunk are staged once for the four waves: wave w fetches the entries 16 w .. 16 w + 15, four channels a lane
  const uint32_t fe = 16u * (uint32_t)w + ((uint32_t)lane >> 2), fc = 4u * ((uint32_t)lane & 3u);

  for (int c0 = 0; c0 < C; c0 += FEAT_BLOCK) {
    if (c0 != 0) __syncthreads();  // (the previous block's last flush read sid / sco / sacc; this block's first chunk writes them)
    float gF[FEAT_BLOCK];
#pragma unroll
    for (int k = 0; k < FEAT_BLOCK; ++k) {
      const float v = f.dL_dimage[(size_t)min(c0 + k, C - 1) * HW + pix];
      gF[k] = (live && c0 + k < C) ? v : 0.f;
    }
    auto fetch = [&](uint32_t id_of_lane) __attribute__((always_inline)) {
      const uint32_t id = (uint32_t)__shfl((int)id_of_lane, (int)fe);
      const float* __restrict__ fr = f.features + (size_t)id * (size_t)C;
      float4 r;
      const int cc = c0 + (int)fc;
      r.x = fr[min(cc, C - 1)];
      r.y = fr[min(cc + 1, C - 1)];
      r.z = fr[min(cc + 2, C - 1)];
      r.w = fr[min(cc + 3, C - 1)];
      r.x = cc < C ? r.x : 0.f;
      r.y = cc + 1 < C ? r.y : 0.f;
      r.z = cc + 2 < C ? r.z : 0.f;
      r.w = cc + 3 < C ? r.w : 0.f;
      return r;
    };
    ChunkWalker<false> walk(a, list_base, tile_max);
    float4 fcur = fetch(walk.cur.id);
    float T = T_final;
    float B_acc = 0.f, last_cdot = 0.f, last_alpha = 0.f;

    auto flush = [&](uint32_t fb, uint32_t fsize) __attribute__((always_inline)) {
      const uint32_t col = (uint32_t)lane & 15u, sub = (uint32_t)lane >> 4;
      // raw moments a geometry column reads (K7's flush): dL_dmean2D (1, 2); opacity 0; conic x / y / w: 3 / 4 / 5
      const uint32_t ia = col == ACC_MEAN2D || col == ACC_MEAN2D + 1u ? 1u
                          : col == ACC_OPACITY ? 0u
                          : col == ACC_CONIC ? 3u : col == ACC_CONIC + 1u ? 4u : col == ACC_CONIC + 3u ? 5u
                          : (uint32_t)FEAT_NM;  // FEAT_NM: the column is not written
#pragma unroll
      for (uint32_t jj = 0; jj < 4u; ++jj) {
        const uint32_t p = 16u * (uint32_t)w + 4u * jj + sub;
        if (16u * (uint32_t)w + 4u * jj >= fsize) break;  // (wave-uniform)
        const bool in = p < fsize;
        float* const row = sacc[fb][in ? p : 0u];
        const bool used = in && ia < (uint32_t)FEAT_NM;
        const float ma = used ? row[ia] : 0.f;
        const float mb = used && ia == 1u ? row[2] : 0.f;
        const float fv = in ? row[FEAT_NM + col] : 0.f;
        const float4 co = sco[fb][in ? p : 0u];  // conic.x, conic.y, conic.z, opacity
        const size_t id = sid[fb][in ? p : 0u];
        float val;
        bool nz;
        if (ia == 1u) {  // backward.cu:545-546
          const bool xcol = col == ACC_MEAN2D;
          const float scale = xcol ? ddelx_dx : ddely_dy, c1 = xcol ? co.x : co.y, c2 = xcol ? co.y : co.z;
          val = -(scale * co.w) * (c1 * ma + c2 * mb);
          nz = ma != 0.f || mb != 0.f;
        } else {  // backward.cu:549-551: -0.5 o t; opacity (:554): the moment itself
          const bool conic = ia >= 3u && ia <= 5u;
          val = conic ? (-0.5f * co.w) * ma : ma;
          nz = ma != 0.f;
        }
        if (used && nz) unsafeAtomicAdd(&a.acc[id * ACC_ROW + col], val);
        if (in && fv != 0.f && c0 + (int)col < C) unsafeAtomicAdd(&f.dL_dfeatures[id * (size_t)C + (size_t)c0 + col], fv);
        if (in) {  // (every read of this instruction precedes it: one wave, program order)
          row[col] = 0.f;
          if (col < (uint32_t)(FEAT_NM + FEAT_BLOCK - 16)) row[16u + col] = 0.f;
        }
      }
    };

    uint32_t pend_size = 0u;
    for (; walk.valid(); walk.advance()) {
      const uint32_t csize = walk.chunk_size();
      const uint32_t cb = walk.chunk & 1u;
      if (w == 0 && (uint32_t)lane < csize) {
        sid[cb][lane] = walk.cur.id;
        sco[cb][lane] = walk.cur.r0;
      }
      *reinterpret_cast<float4*>(&sfeat[cb][fe][fc]) = fcur;
      fcur = fetch(walk.nxt.id);  // (the next chunk's, in flight through this chunk's group loop)
      const uint32_t pos = walk.lane_pos();
      const uint32_t chunk_lo = tile_max - min(tile_max, (walk.chunk + 1u) * (uint32_t)WAVE);
      const uint64_t live_m = __ballot(last_contributor > chunk_lo);
      bool keep = false;
      if (live_m != 0) keep = chunk_cull(live_m, qx0, qy0, ((uint32_t)lane < csize) && (pos < maxc), walk.cur);
      const uint64_t m = __ballot(keep);
      const uint32_t cnt = (uint32_t)__popcll(m);
      const uint32_t cnt4 = (cnt + GROUP - 1) & ~(uint32_t)(GROUP - 1);
      if (keep) {
        const uint32_t slot = (uint32_t)__popcll(m & lt_mask);
        s0[w][slot] = make_float4(-0.5f * walk.cur.r0.x, -walk.cur.r0.y, -0.5f * walk.cur.r0.z, walk.cur.r0.w);
        // .z: the entry's index inside the chunk (= the lane that holds it): its LDS accumulator slot and feature row
        s1[w][slot] = make_float4(walk.cur.r1.x, walk.cur.r1.y, __uint_as_float((uint32_t)lane), __uint_as_float(pos));
      }
      if ((uint32_t)lane >= cnt && (uint32_t)lane < cnt4) {
        s0[w][lane] = make_float4(0.f, 0.f, 0.f, 0.f);  // null entry: alpha 0 => never contributes
        s1[w][lane] = make_float4(0.f, 0.f, __uint_as_float(0u), __uint_as_float(0xffffffffu));
      }
      __syncthreads();  // (A) the chunk's features (and sid / sco) are staged for the four waves
      if (pend_size != 0u) flush(cb ^ 1u, pend_size);
      pend_size = csize;

      for (uint32_t j = 0; j < cnt4; j += GROUP) {
        float G[GROUP], al[GROUP], dxs[GROUP], dys[GROUP];
        bool contrib[GROUP];
        uint32_t cslot[GROUP];
        bool any = false;
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
          const float4 g = s1[w][j + u];
          const float4 co = s0[w][j + u];
          cslot[u] = __float_as_uint(g.z);
          const uint32_t c = __float_as_uint(g.w);
          dxs[u] = g.x - pfx;
          dys[u] = g.y - pfy;
          const float power = blend_power_prescaled(co.x, co.y, co.z, dxs[u], dys[u]);
          G[u] = blend_exp<FAST>(power);
          al[u] = fminf(0.99f, co.w * G[u]);
          contrib[u] = (c < last_contributor) && !(power > 0.0f) && !(al[u] < 1.0f / 255.0f);
          any = any || contrib[u];
        }
        if (!__any(any)) continue;  // wave-uniform

        float v[FEAT_NM][GROUP], mD[GROUP], cdots[GROUP];
        {
#pragma clang fp contract(fast)  // gradients are tolerance-checked (<= 1e-5), not bit-compared
          // cdot = sum_c f_c gF_c of the four entries, one entry's 16 staged features in registers at a time: the next
          // entry's row address is pinned behind this entry's sum (all four rows in flight at once are 64 registers)
#pragma unroll
          for (int u = 0; u < GROUP; ++u) {
            const float4* fp = reinterpret_cast<const float4*>(&sfeat[cb][cslot[u]][0]);
            float cdot = 0.f;
#pragma unroll
            for (int k4 = 0; k4 < FEAT_BLOCK / 4; ++k4) {
              const float4 fv = fp[k4];
              cdot += fv.x * gF[4 * k4] + fv.y * gF[4 * k4 + 1] + fv.z * gF[4 * k4 + 2] + fv.w * gF[4 * k4 + 3];
            }
            cdots[u] = cdot;
            if (u + 1 < GROUP) asm volatile("" : "+v"(cdots[u]), "+v"(cslot[u + 1]));
          }
#pragma unroll
          for (int u = 0; u < GROUP; ++u) {
            const bool on = contrib[u];
            const float alpha = on ? al[u] : 0.f;
            // (no background term: the feature image's background is 0)
            const RecStep rs = accum_rec_step(T, B_acc, last_alpha, last_cdot, rcp_refined(1.f - alpha), cdots[u]);
            T = rs.T;
            B_acc = rs.B_acc;
            last_alpha = alpha;
            last_cdot = on ? cdots[u] : last_cdot;
            const float q = on ? G[u] * rs.dL_dalpha : 0.f;
            mD[u] = alpha * T;  // dF_c / df_c (0 for a skipped lane)
            geometry_moments(v, u, q, dxs[u], dys[u]);
          }
        }
        float totg = wave_sum4_pack<FEAT_NM>(v);
        asm volatile("" : "+v"(totg));
        if (g_adds) atomicAdd(&sacc[cb][__float_as_uint(s1[w][j + g_entry].z)][g_term], totg);
        // the 16 feature terms alpha T gF_c of the four entries, eight channels at a time (32 values: one per lane pair)
        float* const frow = &sacc[cb][__float_as_uint(s1[w][j + f_entry].z)][FEAT_NM + f_term];
#pragma unroll
        for (int h = 0; h < FEAT_BLOCK / FEAT_HALF; ++h) {
          float totf = wave_sum4_pack_outer<FEAT_HALF>(mD, gF + FEAT_HALF * h);
          asm volatile("" : "+v"(totf));
          if (f_adds) atomicAdd(frow + FEAT_HALF * h, totf);
        }
      }
      __syncthreads();  // (B) every quadrant's contribution to this chunk is in sacc[cb]
    }
    asm volatile("" ::"v"(walk.nxt.r0.x), "v"(walk.nxt.r1.x), "v"(walk.id_next), "v"(walk.id_next2), "v"(fcur.x), "v"(fcur.y), "v"(fcur.z), "v"(fcur.w));
    if (pend_size != 0u) flush((walk.chunk - 1u) & 1u, pend_size);
  }
}

template <bool FAST>
__global__ void __launch_bounds__(WAVE* BWD_WAVES) __attribute__((amdgpu_waves_per_eu(FEAT_BWD_WAVES_PER_SIMD, FEAT_BWD_WAVES_PER_SIMD)))
feature_backward_kernel(const BlendArgs a, const FeatureArgs f) {
  __shared__ float4 s0[BWD_WAVES][WAVE], s1[BWD_WAVES][WAVE];
  __shared__ __align__(16) float sfeat[2][WAVE][FEAT_BLOCK];  // (sfeat, sid, sco, sacc: double-buffered by chunk parity)
  __shared__ uint32_t sid[2][WAVE];
  __shared__ float4 sco[2][WAVE];
  __shared__ float sacc[2][WAVE][FEAT_LDS_ROW];
  __shared__ uint32_t s_item;
  for (int i = threadIdx.x; i < 2 * WAVE * FEAT_LDS_ROW; i += WAVE * BWD_WAVES) (&sacc[0][0][0])[i] = 0.f;
  __syncthreads();
  // item-granular queue, as K7: queue x (one per XCD) owns items x, x + 8, ... of the backward's work list
  const uint32_t x = xcc_id() & 7u;
  const uint32_t nwork = a.bwd_meta[0];
  const uint32_t n_x = nwork > x ? (nwork - x + 7u) / 8u : 0u;
  uint32_t* head = a.queue + x * QUEUE_STRIDE;
  // (always_inline: called, the item function would receive the argument blocks through scratch memory)
  auto run_tile = [&](uint32_t index) __attribute__((always_inline)) {
    uint4 item = load_backward_item(a, index);
    item.z = min(item.z, item.w);  // (the depths are the forward's own: never beyond the tile's list)
    feature_backward_tile<FAST>(a, f, item, s0, s1, sfeat, sid, sco, sacc);
  };
  uint32_t x0, base;
  const uint32_t q0 = first_item_of_block((uint32_t)a.units, x0, base);
  {
    const uint32_t n0 = nwork > x0 ? (nwork - x0 + 7u) / 8u : 0u;
    if (q0 < n0) run_tile(x0 + 8u * q0);
  }
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_item = base + __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t q = s_item;
    if (q >= n_x) break;
    run_tile(x + 8u * q);
  }
  if (a.self_reset && threadIdx.x == 0) retire_queue(a.queue);
}

// ----------------------------------------------------------------------------------
// The depth-distortion image (gsr_blend_forward_distortion) and its backward (gsr_blend_backward_distortion): the
// regulariser of Mip-NeRF 360 / 2DGS, per pixel D = 1/2 sum_{i != j} w_i w_j (m_i - m_j)^2 = A M2 - M1^2 with w = alpha T,
// A = sum w, M1 = sum w m, M2 = sum w m^2 over the entries the colour image blends.  No reference counterpart.
// m is the entry's view-space depth z (rec1.z, what the depth image blends), or 2DGS's mapping f (z - n) / ((f - n) z) of it.
// D does not change under m -> m - m0: the moments are accumulated of m' = m - m(z0), z0 the depth of the pixel's FIRST
// blended entry, formed from the difference of the z's -- linear: z - z0; mapped: kappa (z - z0) / (z0 z), kappa = f n / (f - n)
// -- so that A M2' - M1'^2 does not cancel on a thin surface far from the camera (the unshifted float32 moments lose D
// entirely at depth 50, spread 0.05).  One code path for both depths: m' = (kz0 (z - z0)) rz with
// kz0 = 1, rz = 1 (linear: exact) or kz0 = kappa / z0, rz = 1 / z (mapped).
// The forward saves (z0, A, M1', M2') per pixel; with them the backward needs no second pass:
//   dD/dw_k = m'_k^2 A + M2' - 2 m'_k M1' =: c_k,   dD/dm_k = 2 w_k (m'_k A - M1'),   nothing reaches z0 (shift invariance),
//   dL/dalpha_k = T_k (gD c_k - rec_k): K7's recurrence with the scalar gD c_k in the place of the collapsed colour, background 0.
// What is new beside a view's BlendArgs travels as a second kernel argument, as FeatureArgs does.
// ----------------------------------------------------------------------------------
struct DistortionArgs {
  float* out;               // forward: (H,W), fully written
  float4* moments;          // forward: (H,W) (z0, A, M1', M2'), fully written | null
  const float4* moments_in; // backward: what the forward saved
  const float* dL_dD;       // backward: (H,W), the gradient of `out`
  float kappa;              // mapped depth: f n / (f - n); linear: unused
  int mapped;
};

template <bool FAST>
__device__ __forceinline__ void distortion_forward_item(const BlendArgs& a, const DistortionArgs& f, uint32_t tile, uint32_t quad) {
  PixelWave pw;
  ItemBox box;
  if (!setup_item<1>(a, tile, quad, pw, box)) return;
  (void)box;
  const uint2 range = a.ranges[pw.tile];
  const size_t pix = (size_t)pw.py * a.W + pw.px;
  __shared__ __align__(16) float2 szr[WAVE];  // (z, rz) of the chunk's survivors
  const bool mapped = f.mapped != 0;
  const float kappa = wave_uniform(f.kappa);
  bool have = false;
  float z0 = 0.f, kz0 = 1.0f, A = 0.f, M1 = 0.f, M2 = 0.f;
  walk_front_to_back<FAST>(
      a, pw, range,
      [&](uint32_t slot, const Entry& e) __attribute__((always_inline)) {
        szr[slot] = make_float2(e.r1.z, mapped ? 1.0f / e.r1.z : 1.0f);
      },
      [&](uint32_t j, const bool(&hit)[GROUP], const float(&w)[GROUP]) __attribute__((always_inline)) {
        const float4 p01 = *reinterpret_cast<const float4*>(&szr[j]), p23 = *reinterpret_cast<const float4*>(&szr[j + 2]);
        const float zs[GROUP] = {p01.x, p01.z, p23.x, p23.z}, rs[GROUP] = {p01.y, p01.w, p23.y, p23.w};
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
          if (hit[u]) {  // the pixel blends the entry: w = alpha T (a lane-masked region, as the feature forward's)
            if (!have) {
              have = true;
              z0 = zs[u];
              if (mapped) kz0 = kappa / z0;
            }
            const float m = (kz0 * (zs[u] - z0)) * rs[u];
            A += w[u];
            M1 = __builtin_fmaf(w[u], m, M1);
            M2 = __builtin_fmaf(w[u] * m, m, M2);
          }
        }
      },
      [](uint32_t) __attribute__((always_inline)) {});
  if (pw.inside) {
    f.out[pix] = __builtin_fmaf(A, M2, -(M1 * M1));
    if (f.moments != nullptr) f.moments[pix] = make_float4(z0, A, M1, M2);
  }
}
template <bool FAST>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
distortion_forward_kernel(const BlendArgs a, const DistortionArgs f) {
  run_work_queue<1>(a, true, [&](uint32_t tile, uint32_t quad, bool empty) __attribute__((always_inline)) {
    if (!empty) {
      distortion_forward_item<FAST>(a, f, tile, quad);
    } else {  // a tile no Gaussian touches: zeros
      for_each_pixel_of_tile(a, tile, [&](size_t pix, size_t) __attribute__((always_inline)) {
        f.out[pix] = 0.f;
        if (f.moments != nullptr) f.moments[pix] = make_float4(0.f, 0.f, 0.f, 0.f);
      });
    }
  });
}

// The distortion backward: K7's workgroup (the four quadrant waves of a tile, or of half a heavy one), walking the first
// n_contrib entries of every pixel back to front from final_T, as the feature backward does: no checkpoints, a work list
// without list segments.  Per entry a wave reduces SEVEN raw moments: K7's six geometry moments of q = G dL/dalpha and the
// depth moment gD 2 w (m' A - M1'); the four waves add them into one LDS row per chunk slot (rows of 9 floats: odd), and the
// flush -- deferred by a chunk -- is ONE memory-side request per (tile, Gaussian) into the columns ACC_MEAN2D, ACC_OPACITY,
// ACC_CONIC and ACC_DEPTH of the Gaussian's accumulator row; the depth column takes the moment times mu = dm/dz, a constant
// of the entry (1, or kappa / z^2).  ACC_COLOR and ACC_ABS2D are not written.
constexpr int DIST_NM = 7;
constexpr int DIST_LDS_ROW = 9;
static_assert(pack_lanes<DIST_NM>().ok, "every moment of every entry reaches a lane");

template <bool FAST>
__device__ __forceinline__ void distortion_backward_tile(const BlendArgs& a, const DistortionArgs& f, const uint4 item,
                                                         float4 (*s0)[WAVE], float4 (*s1)[WAVE], uint32_t (*sid)[WAVE],
                                                         float4 (*sco)[WAVE], float2 (*szr)[WAVE],
                                                         float (*sacc)[WAVE][DIST_LDS_ROW]) {
  const int w = (int)(threadIdx.x >> 6), lane = lane_id();
  constexpr PackLanes tg = pack_lanes<DIST_NM>();
  auto bit = [lane](uint64_t plane) __attribute__((always_inline)) { return (uint32_t)(plane >> (uint32_t)lane) & 1u; };
  const uint32_t g_term = bit(tg.term_bit[0]) | bit(tg.term_bit[1]) << 1 | bit(tg.term_bit[2]) << 2 | bit(tg.term_bit[3]) << 3;
  const uint32_t g_entry = bit(tg.entry_bit[0]) | bit(tg.entry_bit[1]) << 1;
  const bool g_adds = bit(tg.adds) != 0u;
  // the item: a whole tile (wave w = quadrant w) or half of one (K7's item codes; the work list is built without segments)
  uint32_t tile = item.x;
  const bool half_item = (tile & BWD_ITEM_HALF) != 0u;
  const uint32_t part = (tile & BWD_ITEM_PART) ? 1u : 0u;
  tile &= BWD_ITEM_TILE;
  const uint32_t list_base = item.y, tile_max = item.z;
  if (tile_max == 0) return;  // (uniform: nothing of the item's pixels ever contributed)
  PixelWave pw;
  const bool has_pixels = setup_wave(a, tile, half_item ? 2u * part + (uint32_t)(w >> 1) : (uint32_t)w, pw);
  const float pfx = (float)pw.px, pfy = (float)pw.py;
  const float qx0 = (float)(pw.px - (lane & 7)), qy0 = (float)(pw.py - (lane >> 3));
  if (half_item) pw.inside = pw.inside && ((lane >> 5) == (w & 1));
  const bool live = has_pixels && pw.inside;
  // per-pixel inputs: unconditional loads (a lane without a pixel reads pixel 0 and drops the values)
  const size_t pix = live ? (size_t)pw.py * a.W + pw.px : (size_t)0;
  const float T_final_ld = a.final_T[pix];
  const uint32_t n_contrib_ld = a.n_contrib[pix];
  const float4 mom_ld = f.moments_in[pix];
  const float gD_ld = f.dL_dD[pix];
  ChunkWalker<false> walk(a, list_base, tile_max);
  const float T_final = live ? T_final_ld : 0.f;
  const uint32_t last_contributor = live ? n_contrib_ld : 0u;
  const uint32_t maxc = wave_max_u32_dpp(last_contributor);
  const float gD = live ? gD_ld : 0.f;
  const bool mapped = f.mapped != 0;
  const float kappa = wave_uniform(f.kappa);
  const float z0 = live ? mom_ld.x : 0.f, A = live ? mom_ld.y : 0.f, M1 = live ? mom_ld.z : 0.f, M2 = live ? mom_ld.w : 0.f;
  const float kz0 = mapped ? (z0 > 0.f ? kappa / z0 : 0.f) : 1.0f;  // (z0 = 0: the pixel blends nothing)
  const float nM1x2 = -2.0f * M1;
  const float ddelx_dx = 0.5f * a.W, ddely_dy = 0.5f * a.H;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  float T = T_final;
  float B_acc = 0.f, last_cdot = 0.f, last_alpha = 0.f;

  auto flush = [&](uint32_t fb, uint32_t fsize) __attribute__((always_inline)) {
    const uint32_t col = (uint32_t)lane & 15u, sub = (uint32_t)lane >> 4;
    // raw moments a column reads (K7's flush): dL_dmean2D (1, 2); opacity 0; conic x / y / w: 3 / 4 / 5; depth 6
    const uint32_t ia = col == ACC_MEAN2D || col == ACC_MEAN2D + 1u ? 1u
                        : col == ACC_OPACITY ? 0u
                        : col == ACC_CONIC ? 3u : col == ACC_CONIC + 1u ? 4u : col == ACC_CONIC + 3u ? 5u
                        : col == ACC_DEPTH ? 6u
                        : (uint32_t)DIST_NM;  // DIST_NM: the column is not written
#pragma unroll
    for (uint32_t jj = 0; jj < 4u; ++jj) {
      const uint32_t p = 16u * (uint32_t)w + 4u * jj + sub;
      if (16u * (uint32_t)w + 4u * jj >= fsize) break;  // (wave-uniform)
      const bool in = p < fsize;
      float* const row = sacc[fb][in ? p : 0u];
      const bool used = in && ia < (uint32_t)DIST_NM;
      const float ma = used ? row[ia] : 0.f;
      const float mb = used && ia == 1u ? row[2] : 0.f;
      const float4 co = sco[fb][in ? p : 0u];  // conic.x, conic.y, conic.z, opacity
      const float rz = szr[fb][in ? p : 0u].y;
      const size_t id = sid[fb][in ? p : 0u];
      float val;
      bool nz;
      if (ia == 1u) {  // backward.cu:545-546
        const bool xcol = col == ACC_MEAN2D;
        const float scale = xcol ? ddelx_dx : ddely_dy, c1 = xcol ? co.x : co.y, c2 = xcol ? co.y : co.z;
        val = -(scale * co.w) * (c1 * ma + c2 * mb);
        nz = ma != 0.f || mb != 0.f;
      } else if (ia == 6u) {  // dL/dz = mu dL/dm, mu = dm/dz
        val = mapped ? ((kappa * rz) * rz) * ma : ma;
        nz = ma != 0.f;
      } else {  // backward.cu:549-551: -0.5 o t; opacity (:554): the moment itself
        const bool conic = ia >= 3u && ia <= 5u;
        val = conic ? (-0.5f * co.w) * ma : ma;
        nz = ma != 0.f;
      }
      if (used && nz) unsafeAtomicAdd(&a.acc[id * ACC_ROW + col], val);
      if (in && col < (uint32_t)DIST_NM) row[col] = 0.f;  // (every read of this instruction precedes it: one wave, program order)
    }
  };

  uint32_t pend_size = 0u;
  for (; walk.valid(); walk.advance()) {
    const uint32_t csize = walk.chunk_size();
    const uint32_t cb = walk.chunk & 1u;
    if (w == 0 && (uint32_t)lane < csize) {
      sid[cb][lane] = walk.cur.id;
      sco[cb][lane] = walk.cur.r0;
      szr[cb][lane] = make_float2(walk.cur.r1.z, mapped ? 1.0f / walk.cur.r1.z : 1.0f);
    }
    const uint32_t pos = walk.lane_pos();
    const uint32_t chunk_lo = tile_max - min(tile_max, (walk.chunk + 1u) * (uint32_t)WAVE);
    const uint64_t live_m = __ballot(last_contributor > chunk_lo);
    bool keep = false;
    if (live_m != 0) keep = chunk_cull(live_m, qx0, qy0, ((uint32_t)lane < csize) && (pos < maxc), walk.cur);
    const uint64_t m = __ballot(keep);
    const uint32_t cnt = (uint32_t)__popcll(m);
    const uint32_t cnt4 = (cnt + GROUP - 1) & ~(uint32_t)(GROUP - 1);
    if (keep) {
      const uint32_t slot = (uint32_t)__popcll(m & lt_mask);
      s0[w][slot] = make_float4(-0.5f * walk.cur.r0.x, -walk.cur.r0.y, -0.5f * walk.cur.r0.z, walk.cur.r0.w);
      // .z: the entry's index inside the chunk (= the lane that holds it): its LDS accumulator slot and its (z, rz)
      s1[w][slot] = make_float4(walk.cur.r1.x, walk.cur.r1.y, __uint_as_float((uint32_t)lane), __uint_as_float(pos));
    }
    if ((uint32_t)lane >= cnt && (uint32_t)lane < cnt4) {
      s0[w][lane] = make_float4(0.f, 0.f, 0.f, 0.f);  // null entry: alpha 0 => never contributes
      s1[w][lane] = make_float4(0.f, 0.f, __uint_as_float(0u), __uint_as_float(0xffffffffu));
    }
    __syncthreads();  // (A) the chunk's sid / sco / szr and this wave's survivors are staged
    if (pend_size != 0u) flush(cb ^ 1u, pend_size);
    pend_size = csize;

    for (uint32_t j = 0; j < cnt4; j += GROUP) {
      float G[GROUP], al[GROUP], dxs[GROUP], dys[GROUP], ms[GROUP];
      bool contrib[GROUP];
      bool any = false;
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        const float4 g = s1[w][j + u];
        const float4 co = s0[w][j + u];
        const float2 zr = szr[cb][__float_as_uint(g.z)];
        const uint32_t c = __float_as_uint(g.w);
        dxs[u] = g.x - pfx;
        dys[u] = g.y - pfy;
        ms[u] = (kz0 * (zr.x - z0)) * zr.y;
        const float power = blend_power_prescaled(co.x, co.y, co.z, dxs[u], dys[u]);
        G[u] = blend_exp<FAST>(power);
        al[u] = fminf(0.99f, co.w * G[u]);
        contrib[u] = (c < last_contributor) && !(power > 0.0f) && !(al[u] < 1.0f / 255.0f);
        any = any || contrib[u];
      }
      if (!__any(any)) continue;  // wave-uniform

      float v[DIST_NM][GROUP];
      {
#pragma clang fp contract(fast)  // gradients are tolerance-checked, not bit-compared
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
          const bool on = contrib[u];
          const float alpha = on ? al[u] : 0.f;
          const float mk = on ? ms[u] : 0.f;  // (a skipped entry's depth never enters the recurrence)
          const float cdot = gD * (mk * (mk * A + nM1x2) + M2);  // gD c_k
          const RecStep rs = accum_rec_step(T, B_acc, last_alpha, last_cdot, rcp_refined(1.f - alpha), cdot);
          T = rs.T;
          B_acc = rs.B_acc;
          last_alpha = alpha;
          last_cdot = on ? cdot : last_cdot;
          const float q = on ? G[u] * rs.dL_dalpha : 0.f;
          geometry_moments(v, u, q, dxs[u], dys[u]);
          v[6][u] = (2.0f * gD) * ((alpha * T) * (mk * A - M1));  // gD dD/dm_k (0 for a skipped lane: alpha = 0)
        }
      }
      float tot = wave_sum4_pack<DIST_NM>(v);
      asm volatile("" : "+v"(tot));
      if (g_adds) atomicAdd(&sacc[cb][__float_as_uint(s1[w][j + g_entry].z)][g_term], tot);
    }
    __syncthreads();  // (B) every quadrant's contribution to this chunk is in sacc[cb]
  }
  asm volatile("" ::"v"(walk.nxt.r0.x), "v"(walk.nxt.r1.x), "v"(walk.id_next), "v"(walk.id_next2));
  if (pend_size != 0u) flush((walk.chunk - 1u) & 1u, pend_size);
}

template <bool FAST>
__global__ void __launch_bounds__(WAVE* BWD_WAVES) __attribute__((amdgpu_waves_per_eu(4, 4)))
distortion_backward_kernel(const BlendArgs a, const DistortionArgs f) {
  __shared__ float4 s0[BWD_WAVES][WAVE], s1[BWD_WAVES][WAVE];
  __shared__ uint32_t sid[2][WAVE];  // (sid, sco, szr, sacc: double-buffered by chunk parity)
  __shared__ float4 sco[2][WAVE];
  __shared__ float2 szr[2][WAVE];
  __shared__ float sacc[2][WAVE][DIST_LDS_ROW];
  __shared__ uint32_t s_item;
  for (int i = threadIdx.x; i < 2 * WAVE * DIST_LDS_ROW; i += WAVE * BWD_WAVES) (&sacc[0][0][0])[i] = 0.f;
  __syncthreads();
  // item-granular queue, as K7: queue x (one per XCD) owns items x, x + 8, ... of the backward's work list
  const uint32_t x = xcc_id() & 7u;
  const uint32_t nwork = a.bwd_meta[0];
  const uint32_t n_x = nwork > x ? (nwork - x + 7u) / 8u : 0u;
  uint32_t* head = a.queue + x * QUEUE_STRIDE;
  auto run_tile = [&](uint32_t index) __attribute__((always_inline)) {
    uint4 item = load_backward_item(a, index);
    item.z = min(item.z, item.w);  // (the depths are the forward's own: never beyond the tile's list)
    distortion_backward_tile<FAST>(a, f, item, s0, s1, sid, sco, szr, sacc);
  };
  uint32_t x0, base;
  const uint32_t q0 = first_item_of_block((uint32_t)a.units, x0, base);
  {
    const uint32_t n0 = nwork > x0 ? (nwork - x0 + 7u) / 8u : 0u;
    if (q0 < n0) run_tile(x0 + 8u * q0);
  }
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_item = base + __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t q = s_item;
    if (q >= n_x) break;
    run_tile(x + 8u * q);
  }
  if (a.self_reset && threadIdx.x == 0) retire_queue(a.queue);
}

// Work list of the backward blend: tiles ordered by the work the FORWARD blend measured for them (entries evaluated,
// summed over the four quadrants; the backward revisits the same (pixel, entry) pairs), heaviest first, in buckets of
// 16 entries; tiles in which the forward evaluated nothing have no contributor anywhere and are dropped.  The list
// length, which orders the forward's own work list, is a poor predictor because of early termination.
// One 1024-thread block (T is a few thousand); the order inside a bucket depends on LDS-atomic timing: scheduling
// only, never results.
constexpr int BWD_BUCKETS = 256;
// A tile whose work comes close to a workgroup's fair share of the whole launch would decide the run time on its own
// (the kernel ends with its longest tile: measured 505 K of 509 K cycles).  Such tiles are cut into two items, each
// a workgroup that covers TWO quadrants with two waves per quadrant (8x4 pixels per wave): half the tile per
// workgroup, and the finer culling shortens the waves' lists as well.  `workgroups` = size of the launch.
// GSR_FLAG_CLEAR_GRADS: the four arrays the blend backward accumulates into are cleared by EXTRA blocks of this launch
// (blocks 1 .. gridDim.x - 1; block 0 is the work list): the list is one block of dependent round trips during which the
// rest of the chip idles.  Measured: work list 8.2 us + a separate fill of 44 bytes per Gaussian 8.9 us -> 14 us together
// (the fill runs at 3.1 TB/s here against 4.9 TB/s alone), and one launch less between the forward and the backward.
struct ClearArgs {
  float* ptr[4];
  long long n[4];  // floats
};
template <bool SEG>
__global__ void __launch_bounds__(1024) backward_worklist_kernel(int T, const uint32_t* __restrict__ est,
                                                                uint32_t* __restrict__ order, uint32_t* __restrict__ meta,
                                                                uint32_t workgroups, int allow_halves,  // allow_halves: 0, or the threshold in 1/8 of a fair share
                                                                const ClearArgs clear, const uint32_t* __restrict__ tile_maxc,
                                                                const uint32_t* __restrict__ ck_table,
                                                                const uint32_t* __restrict__ ck_work, const CkTable ckp,
                                                                uint32_t slots,   // checkpoint slots in use per tile (<= CK_MAX)
                                                                int seg_share) {  // 0, or the threshold in 1/8 of a fair share
  if (blockIdx.x != 0) {
    const long long nb = (long long)gridDim.x - 1, b = (long long)blockIdx.x - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float* const p = clear.ptr[k];
      const long long n = clear.n[k];
      if (p == nullptr || n <= 0) continue;
      // 16-byte stores over the aligned middle, scalar stores at the two ends
      const long long head = min(n, (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / 4u));
      const long long n4 = (n - head) / 4;
      typedef float f4 __attribute__((ext_vector_type(4)));
      f4* const q = reinterpret_cast<f4*>(p + head);
      const f4 z = {0.f, 0.f, 0.f, 0.f};
      // consecutive blocks take consecutive 64 KB pieces (4 x 16 KB per thread block and round), four stores in flight per thread
      for (long long i0 = b * 4096; i0 < n4; i0 += nb * 4096) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const long long i = i0 + u * 1024 + threadIdx.x;
          if (i < n4) q[i] = z;
        }
      }
      if (b == 0) {
        for (long long i = threadIdx.x; i < head; i += 1024) p[i] = 0.f;
        for (long long i = head + 4 * n4 + threadIdx.x; i < n; i += 1024) p[i] = 0.f;
      }
    }
    return;
  }
  // (BWD_SUB counters per bucket, chosen by the lane: see tile_worklist_kernel in gsr_binning.hip)
  constexpr int BWD_SUB = 16, NCNT = (BWD_BUCKETS + 1) * BWD_SUB;
  constexpr int CK_TILES_MAX = CK_TILES_CAP;  // (ck_tiles(T) at most: the ranks of Image::ck_table)
  static_assert(BWD_BUCKETS <= 256, "a segment item's bucket is cached in one byte");
  __shared__ uint32_t cnt[NCNT];
  __shared__ uint32_t smem[1024 / 64 + 1];
  __shared__ uint32_t s_threshold, s_seg_threshold, s_ncand;
  // List segments (SEG): what the three passes below need of a cut tile, by the tile's checkpoint rank -- filled ONCE
  // (round 6; rounds 4-5 re-read the tile's row of ck_work in every pass, one dependent round trip per tile and pass in a
  // kernel that is ONE block between two blend kernels: 21 us where the kernel without segments takes 9).
  constexpr uint32_t SEG_CUT = 0x80000000u;
  __shared__ uint32_t s_tile[SEG ? CK_TILES_MAX : 1];         // tile | strides << 20 | SEG_CUT; 0 = the rank's tile is no candidate
  __shared__ uint16_t s_queue[SEG ? CK_TILES_MAX : 1];        // ranks of the candidates
  __shared__ uint8_t s_bucket[SEG ? CK_TILES_MAX : 1][CK_MAX];  // bucket of every stride's item
  const uint32_t sub = threadIdx.x & (BWD_SUB - 1);
  for (int i = threadIdx.x; i < NCNT; i += 1024) cnt[i] = 0;
  if (SEG) {
    for (int i = threadIdx.x; i < CK_TILES_MAX; i += 1024) s_tile[i] = 0u;
    if (threadIdx.x == 0) s_ncand = 0u;
  }
  // The kernel is one block between the forward and the backward blend, i.e. a chain of dependent round trips: the
  // forward's counts are fetched ONCE (all loads of a thread in flight together; images of up to 1024 * EST_REG tiles keep
  // them in registers, larger ones re-read) and the counters are scanned by one block scan.
  constexpr int EST_REG = 8;
  const bool in_regs = T <= 1024 * EST_REG;
  uint4 er[EST_REG];
  uint32_t deep[EST_REG];  // how far the backward walks the tile (0 unless deeper than one checkpoint stride)
  uint32_t rank[EST_REG];  // the tile's checkpoint rank (CK_NONE: it owns no slots)
  const uint32_t stride = slots >= 2u ? ckp.pos(1u) : 0u;  // the first checkpoint: a tile the backward walks no deeper is never cut
  const bool segments = SEG && ck_table != nullptr && tile_maxc != nullptr && ck_work != nullptr && stride != 0u && slots >= 2u && seg_share > 0;
#pragma unroll
  for (int j = 0; j < EST_REG; ++j) {
    const int t = (int)threadIdx.x + 1024 * j;
    er[j] = (in_regs && T > 0) ? reinterpret_cast<const uint4*>(est)[t < T ? t : T - 1] : make_uint4(0u, 0u, 0u, 0u);
    deep[j] = (in_regs && segments && T > 0) ? tile_maxc[t < T ? t : T - 1] : 0u;
    rank[j] = (in_regs && segments && T > 0) ? ck_table[t < T ? t : T - 1] : CK_NONE;
    if (t >= T) {
      er[j] = make_uint4(0u, 0u, 0u, 0u);
      deep[j] = 0u;
      rank[j] = CK_NONE;
    }
  }
  // total work -> the weight above which a tile is cut
  uint32_t mine = 0;
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < EST_REG; ++j) mine += er[j].x + er[j].y + er[j].z + er[j].w;
  } else {
    for (int t = threadIdx.x; t < T; t += 1024) {
      const uint4 e = reinterpret_cast<const uint4*>(est)[t];
      mine += e.x + e.y + e.z + e.w;
    }
  }
  uint32_t total;
  (void)block_excl_scan_u32<1024>(mine, &total, smem);
  if (threadIdx.x == 0) {
    s_threshold = allow_halves ? max(64u, (uint32_t)((uint64_t)total * (uint32_t)allow_halves / (8u * max(workgroups, 1u)))) : 0xffffffffu;
    s_seg_threshold = segments ? max(64u, (uint32_t)((uint64_t)total * (uint32_t)seg_share / (8u * max(workgroups, 1u)))) : 0xffffffffu;
  }
  __syncthreads();
  const uint32_t threshold = s_threshold, seg_threshold = s_seg_threshold;
  auto bucket_of = [](uint32_t w) -> uint32_t {
    if (w == 0) return BWD_BUCKETS;  // nothing to do: after the end of the list
    return (uint32_t)(BWD_BUCKETS - 1) - min((w - 1u) / 16u, (uint32_t)(BWD_BUCKETS - 1));
  };
  // every tile of this thread with what the passes need of it: fn(tile, its four counts, its checkpoint rank, its depth)
  auto for_each_tile = [&](auto&& fn) {
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < EST_REG; ++j) {
        const int t = (int)threadIdx.x + 1024 * j;
        if (t < T) fn(t, er[j], rank[j], deep[j]);
      }
    } else {
      for (int t = threadIdx.x; t < T; t += 1024)
        fn(t, reinterpret_cast<const uint4*>(est)[t], segments ? ck_table[t] : CK_NONE, segments ? tile_maxc[t] : 0u);
    }
  };
  if (segments) {
    // List segments: a tile the backward walks deeper than one checkpoint stride AND whose work is a sizeable share of a
    // workgroup's becomes one item per stride, provided it owns checkpoint slots (the forward then left the state every
    // segment starts from); the items run in different workgroups at the same time.  (a) the candidates are queued; (b) ONE
    // thread per candidate fetches the tile's counts and its whole row of ck_work at once -- entry k: what the forward had
    // evaluated in the tile when it reached checkpoint k, so stride j holds entries k = j .. j + 1 of it: the front strides
    // hold most of the work, the deep positions of a list are walked for a few stragglers -- and decides: a cut only pays
    // if it really divides the work (a tile whose largest stride holds more than 4/5 of it stays whole).
    for_each_tile([&](int t, const uint4 e, uint32_t rk, uint32_t dp) {
      const uint32_t w = e.x + e.y + e.z + e.w;
      if (rk == CK_NONE || rk >= (uint32_t)CK_TILES_MAX || w < seg_threshold || dp <= stride) return;
      uint32_t ns = 1u;  // segments the backward's walk reaches into: one more than the checkpoints in front of its end
#pragma unroll
      for (uint32_t k = 1u; k < (uint32_t)CK_MAX; ++k) ns += (k < slots && ckp.pos(k) < dp) ? 1u : 0u;
      s_tile[rk] = (uint32_t)t | (ns << 20);
      s_queue[atomicAdd(&s_ncand, 1u)] = (uint16_t)rk;
    });
    __syncthreads();
    const uint32_t ncand = s_ncand;
    for (uint32_t c = threadIdx.x; c < ncand; c += 1024) {
      const uint32_t rk = s_queue[c], tt = s_tile[rk];
      const uint32_t t = tt & BWD_ITEM_TILE, ns = (tt >> 20) & 31u;
      const uint4 e = reinterpret_cast<const uint4*>(est)[t];
      const uint32_t* row = ck_work + (size_t)t * slots;
      uint32_t at[CK_MAX + 1];  // at[j]: entries evaluated in front of stride j (at[0] = 0, at[j >= ns] = the tile's total)
#pragma unroll
      for (uint32_t j = 1; j < (uint32_t)CK_MAX; ++j) at[j] = row[min(j, slots - 1u)];  // (unconditional: all in flight)
      const uint32_t w = e.x + e.y + e.z + e.w;
      at[0] = 0u;
      at[CK_MAX] = w;
#pragma unroll
      for (uint32_t j = 1; j < (uint32_t)CK_MAX; ++j) at[j] = j < ns ? min(at[j], w) : w;
      uint32_t largest = 0u;
#pragma unroll
      for (uint32_t j = 0; j < (uint32_t)CK_MAX; ++j) {
        const uint32_t sw = max(at[j + 1] > at[j] ? at[j + 1] - at[j] : 0u, 1u);
        if (j < ns) {
          largest = max(largest, sw);
          s_bucket[rk][j] = (uint8_t)bucket_of(sw);
        }
      }
      if (ns > 1u && (uint64_t)largest * 5u <= (uint64_t)w * 4u) s_tile[rk] = tt | SEG_CUT;
    }
    __syncthreads();
  }
  // strides of a tile that is cut (0: it is not)
  auto strides_of = [&](uint32_t rk) -> uint32_t {
    if (!segments || rk == CK_NONE || rk >= (uint32_t)CK_TILES_MAX) return 0u;
    const uint32_t tt = s_tile[rk];
    return (tt & SEG_CUT) ? ((tt >> 20) & 31u) : 0u;
  };
  for_each_tile([&](int t, const uint4 e, uint32_t rk, uint32_t) {
    const uint32_t w = e.x + e.y + e.z + e.w;
    const uint32_t ns = strides_of(rk);
    if (ns != 0u) {
      for (uint32_t j = 0; j < ns; ++j) atomicAdd(&cnt[(uint32_t)s_bucket[rk][j] * BWD_SUB + sub], 1u);
    } else if (w >= threshold) {
      atomicAdd(&cnt[bucket_of(e.x + e.y) * BWD_SUB + sub], 1u);
      atomicAdd(&cnt[bucket_of(e.z + e.w) * BWD_SUB + sub], 1u);
    } else {
      atomicAdd(&cnt[bucket_of(w) * BWD_SUB + sub], 1u);
    }
  });
  __syncthreads();
  {  // exclusive scan over the counters in (bucket, sub) order: counts -> cursors (one block scan, CPT counters a thread)
    constexpr int CPT = (NCNT + 1023) / 1024;
    const int i0 = (int)threadIdx.x * CPT;
    uint32_t v[CPT], sum = 0;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      v[j] = i0 + j < NCNT ? cnt[i0 + j] : 0u;
      sum += v[j];
    }
    uint32_t all;
    uint32_t run = block_excl_scan_u32<1024>(sum, &all, smem);
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      if (i0 + j < NCNT) cnt[i0 + j] = run;
      if (i0 + j == BWD_BUCKETS * BWD_SUB) meta[0] = run;  // number of items with work
      run += v[j];
    }
  }
  __syncthreads();
  for_each_tile([&](int t, const uint4 e, uint32_t rk, uint32_t) {
    const uint32_t w = e.x + e.y + e.z + e.w;
    const uint32_t ns = strides_of(rk);
    if (ns != 0u) {
      for (uint32_t j = 0; j < ns; ++j)  // (item code: first and last stride of the run -- here one stride)
        order[atomicAdd(&cnt[(uint32_t)s_bucket[rk][j] * BWD_SUB + sub], 1u)] =
            (uint32_t)t | BWD_ITEM_SEG | (j << BWD_SEG_SHIFT) | (j << BWD_NSEG_SHIFT);
    } else if (w >= threshold) {
      order[atomicAdd(&cnt[bucket_of(e.x + e.y) * BWD_SUB + sub], 1u)] = (uint32_t)t | BWD_ITEM_HALF;
      order[atomicAdd(&cnt[bucket_of(e.z + e.w) * BWD_SUB + sub], 1u)] = (uint32_t)t | BWD_ITEM_HALF | BWD_ITEM_PART;
    } else {
      order[atomicAdd(&cnt[bucket_of(w) * BWD_SUB + sub], 1u)] = (uint32_t)t;
    }
  });
}

// Compute units of the device a launch goes to: the device of the STREAM (a C-ABI caller may hand over a stream of another
// device than the thread's current one), looked up per call, the attribute cached per device ordinal.
static int cus_of_stream(hipStream_t s) {
  static int cache[64] = {};  // 0 = not asked yet (a benign race: every writer stores the same value)
  int dev = 0;
  hipDevice_t sdev = 0;
  if (s != nullptr && hipStreamGetDevice(s, &sdev) == hipSuccess) dev = (int)sdev;
  else (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (cache[dev] == 0) {
    int c = 0;
    (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
    cache[dev] = c > 0 ? c : 256;
  }
  return cache[dev];
}
// Number of persistent waves of a launch: (SIMDs on the device) x (waves per SIMD), 4 by default.
// GSR_BLEND_WAVES_PER_SIMD overrides the default for all blend kernels (the backward is built for exactly 4:
// amdgpu_waves_per_eu).
static int waves_per_simd(bool shared_simds) {
  static const int all = env_knob("GSR_BLEND_WAVES_PER_SIMD", 0, 0, 8);
  // (GSR_FLAG_SHARED_SIMDS: a second stream's kernels run alongside -- 2 waves per SIMD; the environment knob wins)
  return all > 0 ? all : (shared_simds ? 2 : 4);
}
unsigned blend_grid_size(hipStream_t s, bool shared_simds) {
  return (unsigned)cus_of_stream(s) * 4u * (unsigned)waves_per_simd(shared_simds);
}
// Placement units of a launch of `grid` workgroups of `waves_per_wg` waves (see first_item_of_block): SIMDs or CUs; 0 turns
// the assigned first items off (a CU count the fold does not divide).
static unsigned blend_units(unsigned waves_per_wg, unsigned grid, hipStream_t s) {
  const unsigned cus = (unsigned)cus_of_stream(s);
  const unsigned units = waves_per_wg == 1 ? cus * 4u : cus;
  if (units % 8u != 0u || grid % units != 0u) return 0u;
  return units;
}
// The cursors are zero on entry (cleared by tile_worklist_kernel, then by every launch's last workgroup).  A grid too
// large for the retire counters: clear them with a memset before the launch instead.
static hipError_t prepare_queue(hipStream_t s, BlendArgs& a, unsigned grid) {
  const bool use_memset = (grid + 63u) / 64u > (unsigned)QUEUE_GROUPS;
  a.self_reset = use_memset ? 0 : 1;
  return use_memset ? hipMemsetAsync(a.queue, 0, sizeof(uint32_t) * QUEUE_STRIDE * QUEUE_LINES, s) : hipSuccess;
}
// Items a quadrant of the forward / trace kernels is cut into (1, 2 or 4): fewer than two quadrant items per persistent
// wave (bounded by the tile count of the image) and the quadrants are cut.
// A render that will see a backward cuts later (round 6, profiles/r06_s_forward_split.md): the cut costs the BACKWARD --
// a quadrant's work estimate is then the largest count among its sub-items, the tile's checkpoint row their sum, and
// the backward's work list orders and cuts by both -- 5-35 % of K7 on images of 320 x 320 .. 720 x 720, more than the
// forward gains.  Forward-only renders keep the cut that is best for the forward alone.
static int forward_split(unsigned grid, unsigned quads, bool for_backward) {
  if (for_backward) return quads > grid ? 1 : (4u * quads > grid ? 2 : 4);
  return quads >= 2u * grid ? 1 : (quads >= grid ? 2 : 4);
}
// What the three persistent launches share: the grid in workgroups of `waves_per_wg` waves (handed back), the queue's
// cursors and the placement units.
static inline __attribute__((always_inline)) hipError_t persistent_launch(hipStream_t s, BlendArgs& a, unsigned waves_per_wg, unsigned* grid) {
  *grid = blend_grid_size(s, a.shared_simds != 0) / waves_per_wg;
  a.units = (int)blend_units(waves_per_wg, *grid, s);
  return prepare_queue(s, a, *grid);
}
// Run-time choices as the compile-time arguments of a generic lambda: with_constants(f, fast, OneOf<1, 2, 4>{split}) calls
// f(std::bool_constant<fast>{}, std::integral_constant<int, split>{}); an int that is none of the listed values: no call.
template <int... Vs> struct OneOf { int v; };
template <class F> static void with_constants(F f) { f(); }
template <class F, class... Rest> static void with_constants(F f, bool v, Rest... rest);
template <class F, int V, int... Vs, class... Rest> static void with_constants(F f, OneOf<V, Vs...> o, Rest... rest) {
  if (o.v == V) with_constants([&](auto... c) { f(std::integral_constant<int, V>{}, c...); }, rest...);
  else if constexpr (sizeof...(Vs) != 0) with_constants(f, OneOf<Vs...>{o.v}, rest...);
}
template <class F, class... Rest> static void with_constants(F f, bool v, Rest... rest) {
  if (v) with_constants([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_constants([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// Which instantiations of the kernel families are built: the launchers below pick a kernel under these and nowhere else, and
// a call whose choices name none gets hipErrorInvalidValue.  K12 is built for every C, cut and exp mode its launcher lists.
// K6: the profiled kernel in one form; an auxiliary render leaves no checkpoints.
constexpr bool forward_exists(bool PROFILE, bool AUX, int SPLIT, bool FAST, bool CKPT) {
  return PROFILE ? !AUX && SPLIT == 1 && !FAST && !CKPT : !(AUX && CKPT);
}
// K7: a depth backward walks no list segments (the checkpoints hold no depth behind a segment, backward_tile).
constexpr bool backward_exists(bool FAST, bool SEG, bool DEPTH, bool ABS, bool ALPHA) { return !(SEG && DEPTH); }

hipError_t launch_blend_forward(hipStream_t s, BlendArgs a) {
  unsigned grid;
  hipError_t e = persistent_launch(s, a, 1, &grid);
  if (e != hipSuccess) return e;
  const int split = forward_split(grid, 4u * (unsigned)(a.gx * a.gy), a.for_backward != 0);
  const dim3 g(grid), b(WAVE);
  // checkpoints for the backward's list segments: where the caller handed the tables over (gsr_capi.hip: checkpoint_chunks)
  const bool ck = a.ck_table != nullptr && a.ck_chunks > 0 && a.colors3 == nullptr && !a.profile;
  // (a profiled render: the plain kernel, uncut, whatever else the arguments say)
  const bool plain = a.profile == nullptr;
  void (*kernel)(BlendArgs) = nullptr;
  with_constants([&](auto PROFILE, auto AUX, auto SPLIT, auto FAST, auto CKPT) {
    if constexpr (forward_exists(PROFILE, AUX, SPLIT, FAST, CKPT)) kernel = blend_forward_kernel<PROFILE, AUX, SPLIT, FAST, CKPT>;
  }, !plain, plain && a.colors3 != nullptr, OneOf<1, 2, 4>{plain ? split : 1}, plain && a.fast_exp, ck);
  if (kernel == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, g, b, 0, s, a);
  return hipGetLastError();
}
// Host-side launch counts of K7 per instantiation (gsr_debug_blend_backward_launches), index FAST | SEG << 1 | DEPTH << 2 |
// ABS << 3 | ALPHA << 4; relaxed: renders run from several host threads and nothing is ordered by the counts.
static std::atomic<uint64_t> g_bwd_launches[32];
void blend_backward_launch_counts(uint64_t counts[32]) {
  for (int i = 0; i < 32; ++i) counts[i] = g_bwd_launches[i].load(std::memory_order_relaxed);
}
// The backward's own work list, ordered by the work the forward measured (backward_worklist_kernel): `grid` workgroups will
// serve it; `fill_blocks` extra blocks clear what `clear` names; seg_share: 0 -- no list segments --, or the threshold in 1/8 of
// a fair share above which a tile is cut into them (the view's checkpoint tables must be there).
static void launch_backward_worklist(hipStream_t s, const BlendArgs& a, unsigned grid, const ClearArgs& clear, unsigned fill_blocks,
                                     int seg_share) {
  constexpr int halves = 10;  // tiles above 1.25 fair shares are cut in two: measured best (sweep 6..16)
  if (seg_share > 0)
    hipLaunchKernelGGL(backward_worklist_kernel<true>, dim3(1u + fill_blocks), dim3(1024), 0, s, a.gx * a.gy, a.work_est,
                       a.bwd_order, a.bwd_meta, grid, halves, clear, (const uint32_t*)a.tile_maxc,
                       (const uint32_t*)a.ck_table, (const uint32_t*)a.ck_work, a.ck_pos, (uint32_t)a.ck_slots, seg_share);
  else
    hipLaunchKernelGGL(backward_worklist_kernel<false>, dim3(1u + fill_blocks), dim3(1024), 0, s, a.gx * a.gy, a.work_est,
                       a.bwd_order, a.bwd_meta, grid, halves, clear, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, CkTable{}, 0u, 0);
}
hipError_t launch_blend_backward(hipStream_t s, BlendArgs a) {
  // #CUs x 4 workgroups of 4 waves: the same 4 waves per SIMD as the forward
  unsigned grid;
  hipError_t e = persistent_launch(s, a, BWD_WAVES, &grid);
  if (e != hipSuccess) return e;
  bool seg_items = false;  // the work list may hold list-segment items (views whose forward left checkpoints; set below)
  ClearArgs clear = {{nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}};
  if (a.clear_grads) {
    const long long P = a.P;
    clear.ptr[0] = a.acc; clear.n[0] = (long long)ACC_ROW * P;
  }
  if (a.touched != nullptr) {  // the row mask always starts from zero (P bytes rounded up to whole floats: gsr.h asks for the padding)
    clear.ptr[1] = reinterpret_cast<float*>(a.touched); clear.n[1] = ((long long)a.P + 3) / 4;
  }
  if (a.work_est == nullptr || a.work_maxc == nullptr || a.bwd_order == nullptr) return hipErrorInvalidValue;
  {
    const unsigned fill_blocks = a.clear_grads ? 2u * (unsigned)cus_of_stream(s) : (a.touched != nullptr ? 16u : 0u);  // (1 .. 8 per CU: the same 14 us)
    // GSR_BWD_SEG: tiles above this many eighths of a fair share are cut into list segments where the forward left
    // checkpoints (0: never; tests use 1)
    static const int seg_share = env_knob("GSR_BWD_SEG", 5, 0, INT_MAX);
    // (Merging consecutive strides of a cut tile into items of about equal measured work -- the plan of
    //  profiles/r06_k -- was built and swept over eleven workloads at 2 .. 12 sixteenths of a fair share per item: equal at
    //  best, 8-40 % slower where pixels walk deep; removed: profiles/r06_m_fine_checkpoints.md.)
    // (a depth backward: no segments -- the checkpoints hold no depth behind a segment, backward_tile)
    seg_items = a.ck_table != nullptr && a.ck_chunks > 0 && seg_share > 0 && a.dL_ddepth == nullptr;
    launch_backward_worklist(s, a, grid, clear, fill_blocks, seg_items ? seg_share : 0);
  }
  const dim3 g(grid), b(WAVE * BWD_WAVES);
  // (dL_dalpha: gsr_blend_backward_alpha -- the ALPHA twin of whatever the call would launch without it)
  // (abs_grad: GSR_FLAG_ABS_GRAD -- the ABS twins of the three routes, nothing else is instantiated)
  void (*kernel)(BlendArgs) = nullptr;
  int index = 0;
  with_constants([&](auto FAST, auto SEG, auto DEPTH, auto ABS, auto ALPHA) {
    if constexpr (backward_exists(FAST, SEG, DEPTH, ABS, ALPHA)) {
      kernel = blend_backward_kernel<FAST, SEG, DEPTH, ABS, ALPHA>;
      constexpr int of_kernel = FAST | SEG << 1 | DEPTH << 2 | ABS << 3 | ALPHA << 4;
      index = of_kernel;
    }
  }, a.fast_exp != 0, seg_items, a.dL_ddepth != nullptr, a.abs_grad != 0, a.dL_dalpha != nullptr);
  if (kernel == nullptr) return hipErrorInvalidValue;
  g_bwd_launches[index].fetch_add(1, std::memory_order_relaxed);
  hipLaunchKernelGGL(kernel, g, b, 0, s, a);
  return hipGetLastError();
}
// GSR_FLAG_ABS_GRAD: the way of K7's absolute sums out of the accumulator table (gsr_abs_grad_take), between K7 and K8+K9.
// One thread per Gaussian: a row K7 marked gives up its columns ACC_ABS2D, + 1 and gets zeros back -- K8+K9 then finds the
// table of a backward without the flag (its `dirty` test does not look at these columns: left in the row they would stay
// behind whenever the signed sums cancel) --, every other Gaussian gets three zeros without its row being read.
__global__ void __launch_bounds__(256) abs_grad_take_kernel(int P, float* acc, const uint8_t* touched, float* absgrad) {
  const int g = (int)(blockIdx.x * 256u + threadIdx.x);
  if (g >= P) return;
  float ax = 0.f, ay = 0.f;
  if (touched == nullptr || touched[g] != 0) {
    float2* const p = reinterpret_cast<float2*>(acc + (size_t)g * ACC_ROW + ACC_ABS2D);  // (8-byte aligned: the row is 64-byte aligned)
    const float2 v = *p;
    ax = v.x;
    ay = v.y;
    if (ax != 0.f || ay != 0.f) *p = make_float2(0.f, 0.f);
  }
  absgrad[3 * (size_t)g] = ax;
  absgrad[3 * (size_t)g + 1] = ay;
  absgrad[3 * (size_t)g + 2] = 0.f;
}
hipError_t launch_abs_grad_take(hipStream_t s, int P, float* acc, const uint8_t* touched, float* absgrad) {
  hipLaunchKernelGGL(abs_grad_take_kernel, dim3(((unsigned)P + 255u) / 256u), dim3(256), 0, s, P, acc, touched, absgrad);
  return hipGetLastError();
}
// The alpha image A = 1 - T_final (gsr_alpha_image) from the image state a forward left: one thread per pixel, or per four
// pixels where the pixel count allows whole float4s (the state's arrays are 256-byte aligned; `out` is the caller's).  A
// kernel of its own and not a K6 twin: the auxiliary render and a render served by view reuse get the image from the
// remembered state without a K6 of theirs, and K6's instantiations stay what they are.
__global__ void __launch_bounds__(256) alpha_image_kernel(size_t n, int vec4, const float* __restrict__ final_T,
                                                          float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;  // (n: float4s if vec4 -- uniform --, else pixels)
  if (i >= n) return;
  if (vec4) {
    const float4 t = reinterpret_cast<const float4*>(final_T)[i];
    reinterpret_cast<float4*>(out)[i] = make_float4(1.0f - t.x, 1.0f - t.y, 1.0f - t.z, 1.0f - t.w);
  } else {
    out[i] = 1.0f - final_T[i];
  }
}
hipError_t launch_alpha_image(hipStream_t s, int W, int H, const float* final_T, float* out_alpha) {
  const size_t N = (size_t)W * H;
  const int vec4 = ((N & 3u) == 0 && (((uintptr_t)final_T | (uintptr_t)out_alpha) & 15u) == 0) ? 1 : 0;
  const size_t n = vec4 ? N / 4 : N;
  hipLaunchKernelGGL(alpha_image_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, n, vec4, final_T, out_alpha);
  return hipGetLastError();
}
hipError_t launch_trace_weights(hipStream_t s, BlendArgs a) {
  unsigned grid;
  hipError_t e = persistent_launch(s, a, 1, &grid);
  if (e != hipSuccess) return e;
  const int split = forward_split(grid, 4u * (unsigned)(a.gx * a.gy), false);
  const dim3 g(grid), b(WAVE);
  void (*kernel)(BlendArgs) = nullptr;  // (stays null for a C that is not listed)
  with_constants([&](auto C, auto SPLIT, auto FAST) { kernel = trace_weights_kernel<C, SPLIT, FAST>; },
                 OneOf<1, 2, 3>{a.C}, OneOf<1, 2, 4>{split}, a.fast_exp != 0);
  if (kernel == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, g, b, 0, s, a);
  return hipGetLastError();
}
// K12's sibling (gsr_trace_contributions): the same grid, cut and queue kind; a.C (0 .. 3) and a.image_weights as for K12.
hipError_t launch_trace_contributions(hipStream_t s, BlendArgs a, int64_t* stats, int32_t* top_id, float* top_weight) {
  unsigned grid;
  hipError_t e = persistent_launch(s, a, 1, &grid);
  if (e != hipSuccess) return e;
  const int split = forward_split(grid, 4u * (unsigned)(a.gx * a.gy), false);
  ContribArgs f = {reinterpret_cast<unsigned long long*>(stats), top_id, top_weight};
  void (*kernel)(BlendArgs, ContribArgs) = nullptr;  // (stays null for a C that is not listed)
  with_constants([&](auto C, auto SPLIT, auto FAST) { kernel = trace_contributions_kernel<C, SPLIT, FAST>; },
                 OneOf<0, 1, 2, 3>{a.C}, OneOf<1, 2, 4>{split}, a.fast_exp != 0);
  if (kernel == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE), 0, s, a, f);
  return hipGetLastError();
}

// The feature image and its backward (gsr_blend_forward_features / gsr_blend_backward_features): one launch each, plus the
// backward's own work list -- built WITHOUT list segments and without clears, whatever the colour backward of the view left
// in Image::bwd_order.
hipError_t launch_feature_forward(hipStream_t s, BlendArgs a, const float* features, float* out, int C) {
  unsigned grid;
  hipError_t e = persistent_launch(s, a, 1, &grid);
  if (e != hipSuccess) return e;
  FeatureArgs f = {features, out, nullptr, nullptr, C};
  void (*kernel)(BlendArgs, FeatureArgs) = nullptr;
  with_constants([&](auto FAST) { kernel = feature_forward_kernel<FAST>; }, a.fast_exp != 0);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE), 0, s, a, f);
  return hipGetLastError();
}
hipError_t launch_feature_backward(hipStream_t s, BlendArgs a, const float* features, const float* dL_dimage,
                                   float* dL_dfeatures, int C) {
  // #CUs x 3 workgroups of 4 waves (FEAT_BWD_WAVES_PER_SIMD: what is resident), fewer where the view's launches are smaller
  unsigned grid = min(blend_grid_size(s, a.shared_simds != 0) / BWD_WAVES, (unsigned)cus_of_stream(s) * FEAT_BWD_WAVES_PER_SIMD);
  a.units = (int)blend_units(BWD_WAVES, grid, s);
  hipError_t e = prepare_queue(s, a, grid);
  if (e != hipSuccess) return e;
  if (a.work_est == nullptr || a.work_maxc == nullptr || a.bwd_order == nullptr) return hipErrorInvalidValue;
  launch_backward_worklist(s, a, grid, ClearArgs{{nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}}, 0u, 0);
  FeatureArgs f = {features, nullptr, dL_dimage, dL_dfeatures, C};
  void (*kernel)(BlendArgs, FeatureArgs) = nullptr;
  with_constants([&](auto FAST) { kernel = feature_backward_kernel<FAST>; }, a.fast_exp != 0);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE * BWD_WAVES), 0, s, a, f);
  return hipGetLastError();
}

// The distortion image and its backward (gsr_blend_forward_distortion / gsr_blend_backward_distortion): one launch each, plus
// the backward's own work list, built as the feature backward's.  kappa = f n / (f - n) of the mapped depth, 0: linear.
hipError_t launch_distortion_forward(hipStream_t s, BlendArgs a, float kappa, float* out, float* moments) {
  unsigned grid;
  hipError_t e = persistent_launch(s, a, 1, &grid);
  if (e != hipSuccess) return e;
  DistortionArgs f = {out, reinterpret_cast<float4*>(moments), nullptr, nullptr, kappa, kappa != 0.f ? 1 : 0};
  void (*kernel)(BlendArgs, DistortionArgs) = nullptr;
  with_constants([&](auto FAST) { kernel = distortion_forward_kernel<FAST>; }, a.fast_exp != 0);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE), 0, s, a, f);
  return hipGetLastError();
}
hipError_t launch_distortion_backward(hipStream_t s, BlendArgs a, float kappa, const float* moments, const float* dL_ddistortion) {
  // #CUs x 4 workgroups of 4 waves, as K7
  unsigned grid;
  hipError_t e = persistent_launch(s, a, BWD_WAVES, &grid);
  if (e != hipSuccess) return e;
  if (a.work_est == nullptr || a.work_maxc == nullptr || a.bwd_order == nullptr) return hipErrorInvalidValue;
  launch_backward_worklist(s, a, grid, ClearArgs{{nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}}, 0u, 0);
  DistortionArgs f = {nullptr, nullptr, reinterpret_cast<const float4*>(moments), dL_ddistortion, kappa, kappa != 0.f ? 1 : 0};
  void (*kernel)(BlendArgs, DistortionArgs) = nullptr;
  with_constants([&](auto FAST) { kernel = distortion_backward_kernel<FAST>; }, a.fast_exp != 0);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE * BWD_WAVES), 0, s, a, f);
  return hipGetLastError();
}

}  // namespace gsr
