// gsr_kernels.h -- kernel argument blocks and host-side launchers shared by the translation units.
#pragma once
#include "gsr_common.h"

namespace gsr {

// K1 arguments (preprocess_kernel, gsr_preprocess.hip)
struct PreArgs {
  int P, D, M;
  int antialias;               // GSR_FLAG_ANTIALIAS: the preprocess_kernel<MAIN, true> instantiations (opacity * h in rec0.w)
                               // (in the padding in front of the pointers: the struct's size and layout stay what they were)
  const float* means3D;
  const float* scales;
  float scale_modifier;
  const float* rotations;
  const float* opacities;
  const float* shs;
  const float* cov3D_precomp;
  const float* colors_precomp;
  const float* viewmatrix;
  const float* projmatrix;
  const float* campos;
  int W, H;
  float tan_fovx, tan_fovy, focal_x, focal_y;
  int gx, gy;
  int skip_color;
  int forward_only;  // GSR_FLAG_FORWARD_ONLY: Geom::dcol (read by the backward only) is not written
  int tile_bounds;  // 0: the reference's square of side 2 ceil(3 sigma_max); 1: its intersection with the alpha >= 1/255 box (gsr_set_option)
  int32_t* radii;
  Geom g;
};

// K8+K9 arguments (preprocess_backward_kernel, gsr_preprocess.hip)
struct PreBwdArgs {
  int P, D, M;
  int depth;                   // GSR_FLAG_DEPTH_GRAD: column ACC_DEPTH (dL_ddepth) enters dL_dmeans3D (not with row_state)
                               // (in the padding in front of the pointers: the struct's size and layout stay what they were)
  const float* means3D;
  const int32_t* radii;
  const float* shs;
  const float* scales;
  const float* rotations;
  float scale_modifier;
  uint32_t rec0_lines;         // GSR_FLAG_ANTIALIAS: Geom::rec0 (opacity * h in .w) lies this many 256-byte lines in front of
                               // `clamped`, in the same geometry state; 0 = flag off.  (A 4-byte offset in the padding behind
                               // scale_modifier instead of a pointer: a larger struct moves the hidden kernel arguments, and
                               // with them the code of every existing instantiation)
  const float* cov3D_precomp;  // (P,6) or null: then recomputed from scales / rotations as K1 did (never stored)
  const uint8_t* clamped;
  const float* dcol[3];        // Geom::dcol: d(RGB)/d(dir) left by K1, 3 floats per Gaussian each (read instead of the SH record)
  const float* viewmatrix;
  const float* projmatrix;
  const float* campos;
  float h_x, h_y, tan_fovx, tan_fovy;
  const float* acc;         // (P, ACC_ROW): the blend backward's accumulator rows (dL_dmean2D, dL_dopacity, dL_dconic, dL_dcolor)
  float* acc_clean;         // == acc (GSR_FLAG_ACC_SELF_CLEAN: rows that are not zero are put back to zero) | null
  float* dL_dmean2D;        // (P,3) out: columns ACC_MEAN2D .. + 1 of the rows, z = 0
  float* dL_dopacity;       // (P)   out: column ACC_OPACITY
  float* dL_dcolor;         // (P,3) out | null: columns ACC_COLOR .. + 2 (the gradient of colors_precomp)
  float* dL_dmeans3D;       // (P,3)
  float* dL_dcov3D;         // (P,6)
  float* dL_dsh;            // (P,M,3) | null
  float* dL_drgb;           // (P,3)   | null: the clamp-masked colour gradient, for gsr_sh_grad_compose
  float* dL_dscale;         // (P,3)   | null
  float* dL_drot;           // (P,4)   | null
  uint8_t* row_state;       // (P) | null: gsr_preprocess_backward_rows -- rows that still hold this kernel's zeros are not rewritten
};

// K6 / K7 / K12 arguments (gsr_blend.hip)
struct BlendArgs {
  int W, H, gx, gy;
  const uint32_t* work_order;  // tile ids, longest first, empty tiles last
  const uint32_t* work_meta;   // [0] = number of non-empty tiles
  uint32_t* work_est;          // forward: out, (T,4) evaluated entries per quadrant; null = not recorded
  uint32_t* work_maxc;         // forward: out, (T,4) deepest contributing list position + 1 per quadrant (with work_est)
  uint32_t* bwd_order;         // backward launch: scratch for its own work list (gsr_blend.hip: backward_worklist_kernel)
  uint32_t* bwd_meta;
  uint32_t* queue;             // 8 per-XCD cursors + retire counters of this kind, QUEUE_STRIDE words apart; zero on
                               // entry, and left zero again by the launch's last workgroup
  const uint2* ranges;
  const uint32_t* point_list;
  const float4* rec0;
  const float4* rec1;
  const float4* rec2;
  const float* colors3;        // auxiliary forward render: (P,3) colours blended instead of rec2; null otherwise
  const float* bg;
  float* final_T;
  uint32_t* n_contrib;
  // forward outputs
  union {
    float* out_color;
    const float* dL_dalpha;  // backward: (1,H,W) gradient of the alpha image 1 - final_T (gsr_blend_backward_alpha), or null --
                             // as dL_ddepth below, in the slot of an output only the forward writes
  };
  union {
    float* out_depth;
    const float* dL_ddepth;  // backward: (1,H,W) gradient of out_depth (gsr_blend_backward_depth), or null -- the slot of the
                             // forward-only output, so that the struct (and every kernel's argument layout) keeps its size
  };
  // backward
  const float* dL_dpix;
  float* acc;      // (P, ACC_ROW): one 64-byte row of accumulators per Gaussian (ACC_* columns, gsr_common.h / include/gsr.h)
  uint8_t* touched;  // (P) | null: 1 for every Gaussian whose row this launch adds to (cleared by the launch itself)
  // tracing
  int C;
  const float* image_weights;
  float* weights;
  int32_t* cnt;
  int P;           // number of Gaussians (rows of the backward's accumulator table)
  int clear_grads; // GSR_FLAG_CLEAR_GRADS: the backward clears its accumulator rows itself (launch_blend_backward)
  int fast_exp;    // GSR_FLAG_FAST_EXP: hardware 2^x instead of the specified polynomial (gsr_blend.hip: blend_exp)
  int shared_simds;  // GSR_FLAG_SHARED_SIMDS: 2 persistent waves per SIMD instead of 4 (another stream's kernels run alongside)
  int self_reset;  // the last workgroup to retire clears the queue cursors (default)
  int abs_grad;    // GSR_FLAG_ABS_GRAD: the backward's ABS instantiations (read by launch_blend_backward alone, never by a kernel;
                   // the slot of a field that went away: the struct, and every kernel's argument layout, keeps its size)
  int for_backward; // forward: the render's state will be read by a backward (not GSR_FLAG_FORWARD_ONLY, not an auxiliary render)
  int units;       // placement units (SIMDs or CUs) for the assigned first items, 0 = none; gsr_blend.hip: first_item_of_block
  // forward checkpoints / backward list segments (Image::ck_*); ck_table == null: none (auxiliary render, tracing)
  uint32_t* ck_table;
  uint32_t* ck_work;
  uint32_t* tile_maxc;
  float4* ck_pool;
  int ck_chunks;   // checkpoint stride in 64-entry chunks
  int ck_slots;    // checkpoint slots in use per tile (<= CK_MAX: the stride of the pool's layout)
  CkTable ck_pos;  // list position of every checkpoint, in 64-entry chunks (gsr_common.h; pos[1] == ck_chunks)
  // debug: per-workgroup timing records (4 x u64 each), or null
  uint64_t* profile_items;  // debug (backward): 4 x u64 per (tile, half) after the workgroup records, or null
  uint64_t* profile;
};

hipError_t launch_preprocess(hipStream_t s, const PreArgs& a);
hipError_t launch_mark_visible(hipStream_t s, int P, const float* means3D, const float* view, uint8_t* present);
hipError_t launch_preprocess_backward(hipStream_t s, const PreBwdArgs& a);
hipError_t launch_sh_grad_compose(hipStream_t s, int P, int D, int M, int N, const float* means3D, const float* campos,
                                  const float* dL_drgb, float* dL_dsh);
// "touched rows" exchange (gsr_preprocess.hip): mask of rows with a non-zero entry in any of up to 8 row-major tensors;
// a view's message = header (camera centre, count, compaction block offsets) + packed rows; all views' messages added
// per Gaussian in view order into the dense gradients (dense: means3D, scales, rotations, means2D, opacities, sh | null)
constexpr int VIEW_MSG_ROWS = 1024;  // rows per block of the message's offset table == the compaction's block (gsr_compact.hip)
hipError_t launch_touched_rows(hipStream_t s, int64_t P, int nt, const float* const* data, const int* row_len, uint8_t* mask);
int64_t view_message_words_host(int64_t P, int64_t cap);
hipError_t launch_view_message_header(hipStream_t s, int64_t P, const float* campos, const uint32_t* block_off,
                                      const uint64_t* total, float* msg);
hipError_t launch_view_messages_accumulate(hipStream_t s, int64_t P, int D, int M, int n_views, const float* messages,
                                           int64_t stride_words, int64_t cap, const float* means3D, float* const dense[6],
                                           uint8_t* row_valid);
const uint32_t* compact_block_off_ptr(void* workspace, int64_t P);
hipError_t launch_export_cov3d(hipStream_t s, int P, const float* scales, float scale_modifier, const float* rotations,
                               float* cov3D);
hipError_t launch_export_geom(hipStream_t s, int P, const Geom& g, float* means2D, float* depths, float* rgb,
                              float* conic_opacity, uint32_t* tiles_touched, uint8_t* clamped);
hipError_t launch_depth_passes(hipStream_t s, int P, const Geom& g, int p0, int p1, uint32_t* publish_dst = nullptr,
                               uint32_t publish_seq = 0);
// Legacy pair sort only: the tile rectangles gathered into depth order + the prefix of their tile counts.
hipError_t launch_depth_finish(hipStream_t s, int P, const Geom& g, int passes, int gx);
// Grouped path: the same passes carrying the packed tile rectangle; `last`: pass p1 - 1 is the final one and leaves the
// depth order, the rectangles in that order and every Gaussian's first slot of the emission (no launch_depth_finish).
hipError_t launch_depth_passes_grouped(hipStream_t s, int P, const Geom& g, int p0, int p1, bool last,
                                       uint32_t* publish_dst = nullptr, uint32_t publish_seq = 0);
hipError_t launch_export_keys(hipStream_t s, int64_t R, int W, int H, const Binning& b, const Geom& g, uint64_t* keys);
hipError_t launch_binning(hipStream_t s, int P, int64_t R, int W, int H, const Geom& g, const Binning& b, const Image& im);
// The binning's stable LSD radix sort of (key, value) pairs, for the other translation units (gsr_knn.hip).
void radix_sort_pairs_u32(hipStream_t s, uint32_t* const keys[2], uint32_t* const vals[2], int64_t n, int npass,
                          const int* digit_bits, uint32_t* hist, uint32_t* bin_total, bool iota_first);
// debug (host only): launches of the radix scatter kernels per instantiation in this process (include/gsr.h:
// gsr_debug_sort_launches states the index layout)
void sort_launch_counts(uint64_t counts[24]);
// debug (host only): launches of group_chunk_kernel per instantiation and stage size (gsr_debug_group_launches)
void group_launch_counts(uint64_t counts[16]);
size_t knn_workspace_bytes(int P);
hipError_t launch_knn(hipStream_t s, int P, const float* points, void* workspace, float* out);
hipError_t launch_near_points(hipStream_t s, int n_ref, const float* ref, int n_query, const float* query, float thresh,
                              void* workspace, uint8_t* near, float* nn_dist);
size_t compact_workspace_bytes(int64_t P);
hipError_t launch_compact_plan(hipStream_t s, int64_t P, const uint8_t* keep, void* workspace);
const uint64_t* compact_total_ptr(void* workspace, int64_t P);
// limit: rows the destinations hold (survivors beyond it are dropped); < 0 = unlimited
hipError_t launch_compact_apply(hipStream_t s, int64_t P, const uint8_t* keep, void* workspace, int nt,
                                const gsr_compact_tensor* tensors, int64_t limit = -1);
hipError_t launch_append_rows(hipStream_t s, int64_t P, int64_t n, int nt, const gsr_append_tensor* tensors);
// the densification policy (gsr_densify.hip)
hipError_t launch_densify_stats(hipStream_t s, int64_t P, int V, const float* const* grads, const int32_t* const* radii,
                                float* accum, float* denom, float* max_radii);
size_t densify_workspace_bytes(int64_t P);
void densify_plans(void* workspace, int64_t P, void** clone_plan, void** split_plan);
hipError_t launch_densify_select(hipStream_t s, int64_t P, const float* accum, const float* denom, const uint8_t* mask,
                                 const float* scaling, float max_grad, double max_densify_percent, float t_dense,
                                 void* workspace, uint8_t* clone_sel, uint8_t* split_sel);
const gsr_densify_result* densify_result_ptr(void* workspace, int64_t P);
hipError_t launch_densify_split_xyz(hipStream_t s, int64_t P, const float* xyz, const float* scaling, const float* rotation,
                                    const uint8_t* split_sel, void* split_plan, int64_t n_split, int N, const float* noise,
                                    float* new_xyz);
hipError_t launch_densify_keep(hipStream_t s, int64_t P, const float* opacity, const float* scaling, const float* max_radii,
                               const uint8_t* mask, const uint8_t* drop, float min_opacity, float max_screen, float big_ws,
                               uint8_t* keep);
// the 3DGS-MCMC strategy (gsr_mcmc.hip)
hipError_t launch_mcmc_noise(hipStream_t s, int64_t P, float* xyz, const float* scaling_raw, const float* rotation_raw,
                             const float* opacity_raw, const float* noise, const uint8_t* mask, double k, double x0,
                             double scaler);
size_t mcmc_workspace_bytes(int64_t P);
const gsr_mcmc_record* mcmc_record_ptr(void* workspace, int64_t P);
hipError_t launch_mcmc_sample(hipStream_t s, int64_t P, int64_t n, const float* opacity, const uint8_t* mask,
                              float min_opacity, const float* u, int draws_from_dead, void* workspace, uint8_t* dead_sel,
                              int32_t* dead_idx, int32_t* src, int32_t* count, int32_t* ratio);
hipError_t launch_mcmc_values(hipStream_t s, int64_t P, int64_t n, const int32_t* src, const int32_t* ratio,
                              const float* opacity, const float* scaling_raw, float min_opacity, float* new_opacity_raw,
                              float* new_scaling_raw);
hipError_t launch_mcmc_scatter(hipStream_t s, int64_t P, int64_t n, const int32_t* src, const int32_t* dst_idx,
                               int64_t dst_rows, int nt, const gsr_mcmc_tensor* tensors);
hipError_t launch_adam_step(hipStream_t s, int nt, const gsr_adam_tensor* tensors, long long step, double beta1,
                            double beta2, double eps, const uint8_t* row_mask, const float* row_weight,
                            const uint8_t* grad_valid = nullptr);
hipError_t launch_blend_forward(hipStream_t s, BlendArgs a);
unsigned blend_grid_size(hipStream_t s, bool shared_simds = false);  // persistent waves of a blend launch on the device of stream s
hipError_t launch_blend_backward(hipStream_t s, BlendArgs a);
// debug (host only): launches of K7 per instantiation in this process, index FAST | SEG << 1 | DEPTH << 2 | ABS << 3 | ALPHA << 4
void blend_backward_launch_counts(uint64_t counts[32]);
constexpr uint32_t BWD_ITEM_SEG_BIT = 0x10000000u;  // item code of Image::bwd_order: a list segment (gsr_blend.hip: BWD_ITEM_SEG)
// GSR_FLAG_ABS_GRAD: columns ACC_ABS2D, + 1 of the accumulator rows -> absgrad (P,3), and back to zero (gsr_blend.hip)
hipError_t launch_abs_grad_take(hipStream_t s, int P, float* acc, const uint8_t* touched, float* absgrad);
// the alpha image (accumulated opacity) 1 - final_T of the image state a forward left (gsr_blend.hip)
hipError_t launch_alpha_image(hipStream_t s, int W, int H, const float* final_T, float* out_alpha);
hipError_t launch_trace_weights(hipStream_t s, BlendArgs a);
// contribution statistics (P, 3 + a.C) int64 and the pick buffer of a view (gsr_blend.hip: trace_contributions_kernel)
hipError_t launch_trace_contributions(hipStream_t s, BlendArgs a, int64_t* stats, int32_t* top_id, float* top_weight);
// the feature image (C channels per Gaussian, composited once per 16-channel block) and its backward (gsr_blend.hip)
hipError_t launch_feature_forward(hipStream_t s, BlendArgs a, const float* features, float* out, int C);
hipError_t launch_feature_backward(hipStream_t s, BlendArgs a, const float* features, const float* dL_dimage,
                                   float* dL_dfeatures, int C);
// the depth-distortion image (A M2 - M1^2 of the blended depths, shifted per pixel) and its backward (gsr_blend.hip);
// kappa = f n / (f - n) of the mapped depth, 0 = the linear depth; moments: (H,W) float4, null in a forward without backward
hipError_t launch_distortion_forward(hipStream_t s, BlendArgs a, float kappa, float* out, float* moments);
hipError_t launch_distortion_backward(hipStream_t s, BlendArgs a, float kappa, const float* moments, const float* dL_ddistortion);

// The camera gradient (pose_backward_kernel, gsr_pose.hip): between K7 and K8+K9, from the accumulator rows K7 left
struct PoseArgs {
  int P, D;
  int sh;                      // the view's colours came from SHs (campos is read, dL/dcampos can be non-zero); 0: colors_precomp
  float scale_modifier;
  const float* means3D;
  const int32_t* radii;
  const float* scales;         // with rotations, or null: then cov3D_precomp
  const float* rotations;
  const float* cov3D_precomp;
  const float* viewmatrix;
  const float* projmatrix;
  const float* campos;
  float h_x, h_y, tan_fovx, tan_fovy;
  const float* acc;            // (P, ACC_ROW), read only
  const uint8_t* clamped;      // Geom::clamped
  const float* dcol[3];        // Geom::dcol
  const float4* rec0;          // Geom::rec0 (AA: opacity * h in .w) | null
  float* partials;             // (blocks, POSE_SUMS_PAD): one row of partial sums per block, fully written
};
constexpr int POSE_SUMS = 27;       // 12 dL/dviewmatrix[:, :3] + 12 dL/dprojmatrix[:, (0, 1, 3)] + 3 dL/dcampos
constexpr int POSE_SUMS_PAD = 32;
constexpr int POSE_MAX_BLOCKS = 1024;
constexpr int POSE_OUT = 35;        // viewmatrix 16, projmatrix 16, campos 3
inline int pose_blocks(int P) {
  const int nb = (P + GAUSS_BLOCK - 1) / GAUSS_BLOCK;
  return nb < 1 ? 1 : (nb > POSE_MAX_BLOCKS ? POSE_MAX_BLOCKS : nb);
}
hipError_t launch_pose_backward(hipStream_t s, const PoseArgs& a, bool depth, bool antialias, float* pose_grad);

#if defined(__HIPCC__)
// ----------------------------------------------------------------------------------
// Device helpers of the per-Gaussian kernels (gsr_preprocess.hip: K1, K8+K9; gsr_pose.hip: the camera gradient), here so
// that both translation units evaluate the covariance chain with the same operations.
// ----------------------------------------------------------------------------------
// glm::mat3 semantics (column-major m[col][row]; product evaluated left to right),
// DGR/third_party/glm/glm/detail/type_mat3x3.inl:486-519.
struct M3 {
  float m[3][3];
};
__device__ __forceinline__ M3 mk(float a, float b, float c, float d, float e, float f, float g, float h, float i) {
  M3 r;
  r.m[0][0] = a; r.m[0][1] = b; r.m[0][2] = c;
  r.m[1][0] = d; r.m[1][1] = e; r.m[1][2] = f;
  r.m[2][0] = g; r.m[2][1] = h; r.m[2][2] = i;
  return r;
}
__device__ __forceinline__ M3 mul(const M3& A, const M3& B) {
  M3 R;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) R.m[c][r] = A.m[0][r] * B.m[c][0] + A.m[1][r] * B.m[c][1] + A.m[2][r] * B.m[c][2];
  return R;
}
__device__ __forceinline__ M3 tr(const M3& A) {
  M3 R;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) R.m[c][r] = A.m[r][c];
  return R;
}

struct Cam {
  float view[16];
  float proj[16];
  float campos[3];
};

__device__ __forceinline__ void load_cam(Cam& c, const float* view, const float* proj, const float* campos) {
  // 35 uniform floats: the compiler turns these into scalar (s_load) loads.
#pragma unroll
  for (int i = 0; i < 16; ++i) c.view[i] = view[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) c.proj[i] = proj[i];
  if (campos) {
#pragma unroll
    for (int i = 0; i < 3; ++i) c.campos[i] = campos[i];
  }
}

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// computeCov3D, forward.cu:118-152: Sigma = (S R)^T (S R), upper triangle.  Used by K1 and again by K8+K9 -- the reference
// keeps the six floats in its geometry buffer between the passes (rasterizer_impl.cu:225, 388); recomputing them from
// the 28 bytes of scale and rotation the backward reads anyway saves a 24-byte store and a 24-byte load per Gaussian.
__device__ __forceinline__ void cov3d_from_values(float s0, float s1, float s2, float scale_modifier, const float4& q,
                                                  float (&c3)[6]) {
  M3 S = mk(1, 0, 0, 0, 1, 0, 0, 0, 1);
  S.m[0][0] = scale_modifier * s0;
  S.m[1][1] = scale_modifier * s1;
  S.m[2][2] = scale_modifier * s2;
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  const M3 R = mk(1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                  2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                  2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y));
  const M3 Mm = mul(S, R);
  const M3 Sigma = mul(tr(Mm), Mm);
  c3[0] = Sigma.m[0][0]; c3[1] = Sigma.m[0][1]; c3[2] = Sigma.m[0][2];
  c3[3] = Sigma.m[1][1]; c3[4] = Sigma.m[1][2]; c3[5] = Sigma.m[2][2];
}

// ---- The projection chain, one definition per piece: K1 evaluates it, K8+K9 and the camera gradient evaluate it again and
// differentiate it, and all three must arrive at the same bits.  (Which kernel calls what, and the forms that keep every
// kernel's code what it was: DESIGN.md, profiles/gaussian_chain_shared_isa.md.)
// transformPoint4x3, auxiliary.h:58-66: the view-space mean
__device__ __forceinline__ V3 view_point(const float* view, V3 p) {
  return {view[0] * p.x + view[4] * p.y + view[8] * p.z + view[12], view[1] * p.x + view[5] * p.y + view[9] * p.z + view[13],
          view[2] * p.x + view[6] * p.y + view[10] * p.z + view[14]};
}
// backward.cu:370-377: what the gradient of ndc = p_hom.xy / (p_hom.w + 1e-7) needs of the homogeneous position
struct HomTerms { float m_w, mul1, mul2; };
__device__ __forceinline__ HomTerms hom_backward_terms(const float* proj, V3 m) {
  const float m_hw = proj[3] * m.x + proj[7] * m.y + proj[11] * m.z + proj[15];
  const float m_w = 1.0f / (m_hw + 0.0000001f);
  const float mul1 = (proj[0] * m.x + proj[4] * m.y + proj[8] * m.z + proj[12]) * m_w * m_w;
  const float mul2 = (proj[1] * m.x + proj[5] * m.y + proj[9] * m.z + proj[13]) * m_w * m_w;
  return {m_w, mul1, mul2};
}
// computeCov2D, forward.cu:74-113 / backward.cu:159-190: t = the view-space mean clamped to the 1.3x cone (x_grad_mul,
// y_grad_mul: 0 where the clamp is active), T = W J, cov = the UNDILATED 2D covariance (entries [0][0], [0][1], [1][1]).
struct Cov2D { V3 t; float x_grad_mul, y_grad_mul; M3 J, W, Vrk, T, cov; };
__device__ __forceinline__ Cov2D cov2d_chain(V3 t, const float* view, const float (&c3)[6], float tan_fovx, float tan_fovy,
                                             float focal_x, float focal_y) {
  Cov2D c;
  const float limx = 1.3f * tan_fovx, limy = 1.3f * tan_fovy;
  const float txtz = t.x / t.z, tytz = t.y / t.z;
  t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
  t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
  c.t = t;
  c.x_grad_mul = txtz < -limx || txtz > limx ? 0.f : 1.f;
  c.y_grad_mul = tytz < -limy || tytz > limy ? 0.f : 1.f;
  c.J = mk(focal_x / t.z, 0.0f, -(focal_x * t.x) / (t.z * t.z), 0.0f, focal_y / t.z, -(focal_y * t.y) / (t.z * t.z), 0, 0, 0);
  c.W = mk(view[0], view[4], view[8], view[1], view[5], view[9], view[2], view[6], view[10]);
  c.Vrk = mk(c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]);
  c.T = mul(c.W, c.J);
  c.cov = mul(mul(tr(c.T), tr(c.Vrk)), c.T);
  return c;
}
// Anti-aliasing: r = det(Sigma) / det(Sigma + 0.3 I) from the undilated covariance and the dilated determinant, and the
// opacity factor h; the floor also covers a det(Sigma) that rounds to <= 0 (on it h is a constant: no r-term in the backward)
constexpr float AA_R_FLOOR = 2.5e-5f;
__device__ __forceinline__ float aa_ratio(M3 cov, float det) {
  return (cov.m[0][0] * cov.m[1][1] - cov.m[0][1] * cov.m[0][1]) * (1.f / det);
}
__device__ __forceinline__ float aa_factor(float r) { return sqrtf(fmaxf(AA_R_FLOOR, r)); }

// backward.cu:192-226: the conic's gradient -> dL/d(a, b, c) of the dilated covariance (a b; b c), and through
// cov = T^T Vrk T to dL/dcov3D (dcov: its six entries, left as they are where the reference's denom2inv is zero).
// aa: plus the r-term of the opacity factor, g_opacity = dL/d(o h) and aa_ow = o h (K8+K9's header); aa_h = h as K1 computed it.
struct Cov2DGrad { float da, db, dc, aa_r, aa_h; };
__device__ __forceinline__ Cov2DGrad cov2d_backward(const M3& cov2D, const M3& T, V3 dL_dcon, bool aa, float g_opacity, float aa_ow,
                                                    float (&dcov)[6]) {
  const float ca = cov2D.m[0][0] + 0.3f, cb = cov2D.m[0][1], cc = cov2D.m[1][1] + 0.3f;
  const float denom = ca * cc - cb * cb;
  const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
  Cov2DGrad g = {0, 0, 0};
  g.aa_r = aa ? aa_ratio(cov2D, denom) : 0.f;
  g.aa_h = aa ? aa_factor(g.aa_r) : 1.f;
  if (denom2inv != 0) {
    g.da = denom2inv * (-cc * cc * dL_dcon.x + 2 * cb * cc * dL_dcon.y + (denom - ca * cc) * dL_dcon.z);
    g.dc = denom2inv * (-ca * ca * dL_dcon.z + 2 * ca * cb * dL_dcon.y + (denom - ca * cc) * dL_dcon.x);
    g.db = denom2inv * 2 * (cb * cc * dL_dcon.x - (denom + 2 * cb * cb) * dL_dcon.y + ca * cb * dL_dcon.z);
    if (aa) {
      const float aa_r = g.aa_r;
      if (aa_r > AA_R_FLOOR) {
        const float x = cov2D.m[0][0], y = cov2D.m[1][1], z = cb, w = 0.3f;
        const float dL_dr = g_opacity * aa_ow / (2.f * aa_r);
        const float s = dL_dr * w / (denom * denom);
        g.da += s * (y * y + w * y + z * z);
        g.dc += s * (x * x + w * x + z * z);
        g.db += s * (-2.f * z * (x + y + w));
      }
    }
    const auto& Tm = T.m;
    dcov[0] = (Tm[0][0] * Tm[0][0] * g.da + Tm[0][0] * Tm[1][0] * g.db + Tm[1][0] * Tm[1][0] * g.dc);
    dcov[3] = (Tm[0][1] * Tm[0][1] * g.da + Tm[0][1] * Tm[1][1] * g.db + Tm[1][1] * Tm[1][1] * g.dc);
    dcov[5] = (Tm[0][2] * Tm[0][2] * g.da + Tm[0][2] * Tm[1][2] * g.db + Tm[1][2] * Tm[1][2] * g.dc);
    dcov[1] = 2 * Tm[0][0] * Tm[0][1] * g.da + (Tm[0][0] * Tm[1][1] + Tm[0][1] * Tm[1][0]) * g.db + 2 * Tm[1][0] * Tm[1][1] * g.dc;
    dcov[2] = 2 * Tm[0][0] * Tm[0][2] * g.da + (Tm[0][0] * Tm[1][2] + Tm[0][2] * Tm[1][0]) * g.db + 2 * Tm[1][0] * Tm[1][2] * g.dc;
    dcov[4] = 2 * Tm[0][2] * Tm[0][1] * g.da + (Tm[0][1] * Tm[1][2] + Tm[0][2] * Tm[1][1]) * g.db + 2 * Tm[1][1] * Tm[1][2] * g.dc;
  }
  return g;
}
// backward.cu:247-270: dL/dT (dT0[r] = dL/dT[0][r], dT1 likewise) through T = W J to dL/dJ, dL/dt (off the cone t.xy are constants)
__device__ __forceinline__ V3 chain_dt(Cov2D c, const float (&dT0)[3], const float (&dT1)[3], float h_x, float h_y) {
  const auto& Wx = c.W.m;
  const float dL_dJ00 = Wx[0][0] * dT0[0] + Wx[0][1] * dT0[1] + Wx[0][2] * dT0[2];
  const float dL_dJ02 = Wx[2][0] * dT0[0] + Wx[2][1] * dT0[1] + Wx[2][2] * dT0[2];
  const float dL_dJ11 = Wx[1][0] * dT1[0] + Wx[1][1] * dT1[1] + Wx[1][2] * dT1[2];
  const float dL_dJ12 = Wx[2][0] * dT1[0] + Wx[2][1] * dT1[1] + Wx[2][2] * dT1[2];
  const float tz = 1.f / c.t.z, tz2 = tz * tz, tz3 = tz2 * tz;
  return {c.x_grad_mul * -h_x * tz2 * dL_dJ02, c.y_grad_mul * -h_y * tz2 * dL_dJ12,
          -h_x * tz2 * dL_dJ00 - h_y * tz2 * dL_dJ11 + (2 * h_x * c.t.x) * tz3 * dL_dJ02 + (2 * h_y * c.t.y) * tz3 * dL_dJ12};
}
// backward.cu:228-270: dL/dT (its two non-zero rows) and dL/dt of one Gaussian
struct ChainGrad { float dT0[3], dT1[3]; V3 dt; };  // dL/dT[0][r], dL/dT[1][r]; dL/dt
__device__ __forceinline__ ChainGrad chain_backward(Cov2D c, Cov2DGrad g, float h_x, float h_y) {
  ChainGrad o;
  const auto& Tm = c.T.m;
  const auto& V = c.Vrk.m;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o.dT0[r] = 2 * (Tm[0][0] * V[r][0] + Tm[0][1] * V[r][1] + Tm[0][2] * V[r][2]) * g.da +
               (Tm[1][0] * V[r][0] + Tm[1][1] * V[r][1] + Tm[1][2] * V[r][2]) * g.db;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o.dT1[r] = 2 * (Tm[1][0] * V[r][0] + Tm[1][1] * V[r][1] + Tm[1][2] * V[r][2]) * g.dc +
               (Tm[0][0] * V[r][0] + Tm[0][1] * V[r][1] + Tm[0][2] * V[r][2]) * g.db;
  o.dt = chain_dt(c, o.dT0, o.dT1, h_x, h_y);
  return o;
}
// dnormvdv, auxiliary.h:107-117: the gradient dv of v / |v| taken back to v
__device__ __forceinline__ V3 dnormvdv(V3 v, V3 dv) {
  const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
  const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
  return {((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32,
          (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32,
          (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32};
}
// dL_dRGB with the channels K1 clamped at zero taken out (Geom::clamped, backward.cu:35-38)
__device__ __forceinline__ V3 unclamped_rgb_grad(V3 dL_dRGB, uint8_t cl) {
  dL_dRGB.x *= (cl & 1) ? 0.f : 1.f;
  dL_dRGB.y *= (cl & 2) ? 0.f : 1.f;
  dL_dRGB.z *= (cl & 4) ? 0.f : 1.f;
  return dL_dRGB;
}
// v / |v|: the direction the SH basis is evaluated in (forward.cu:28-29)
__device__ __forceinline__ V3 unit_dir(V3 v) {
  const float len = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
  return {v.x / len, v.y / len, v.z / len};
}
// The real SH basis of computeColorFromSH (forward.cu:20-71, backward.cu:20-139).
constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
__device__ constexpr float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                       -1.0925484305920792f, 0.5462742152960396f};
__device__ constexpr float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f,  -0.4570457994644658f,
                                       0.3731763325901154f,  -0.4570457994644658f, 1.445305721320277f,
                                       -0.5900435899266435f};
#endif  // __HIPCC__

}  // namespace gsr
