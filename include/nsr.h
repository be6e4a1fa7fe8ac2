/*
 * nsr.h -- C ABI of libnsr_hip.so, the MI355X (gfx950) volume-rendering hot path.
 *
 * Drop-in boundary for the two pybind11 extension modules of hkust-vgd/nerfstyle
 *   _raymarching  (raymarching/src/bindings.cpp:5-21, signatures raymarching/src/raymarching.h:6-38)
 *   _gridencoder  (gridencoder/src/bindings.cpp:5-8,  signatures gridencoder/src/gridencoder.h:12-14)
 * and for the third native surface the reference reaches through tinycudann
 *   tcnn.Network  (networks/style_nerf.py:44-98)
 * plus fused entry points that have no reference counterpart (the reference launches
 * march / encode x2 / MLP x4 / exp / cat / composite separately).
 *
 * Contract (same as the reference's):
 *   - plain C, raw DEVICE pointers + explicit sizes + a HIP stream; no torch types;
 *   - the caller allocates every output and every workspace; the library never allocates,
 *     frees or retains device memory and keeps no state between calls (re-entrant, thread-safe).
 *     The one exception is a per-device "attribute already set" flag beside the two kernels that ask
 *     for more than the default LDS (hipFuncSetAttribute is idempotent: a racing second call is harmless);
 *   - no host synchronisation, no host reads of device data, no library calls (round 3: the sample sort
 *     is the library's own, rocPRIM is gone): every call is legal inside hipGraph stream capture;
 *   - returns an int status (0 = ok, <0 = error) and never throws; the reference returns void
 *     and raises c10::Error / std::runtime_error (gridencoder.cu:369,387,414,433,440-487) --
 *     the Python wrappers turn a negative status into RuntimeError.
 *   - pointer arguments marked "host" are read on the host at call time (small tables).
 *
 * Element-type codes (nsr_dtype): the reference dispatches on at::ScalarType
 * (AT_DISPATCH_FLOATING_TYPES_AND_HALF); this ABI passes a code.
 */
#ifndef NSR_H_
#define NSR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *nsr_stream_t; /* a hipStream_t */

enum nsr_status {
    NSR_OK = 0,
    NSR_ERR_INVALID_ARG = -1, /* null pointer, bad size, bad enum */
    NSR_ERR_UNSUPPORTED = -2, /* configuration outside what the kernels are built for */
    NSR_ERR_LAUNCH = -3       /* hipGetLastError() after the launch was not hipSuccess */
};

enum nsr_dtype { NSR_F32 = 0, NSR_F16 = 1, NSR_BF16 = 2 };
enum nsr_activation { NSR_ACT_NONE = 0, NSR_ACT_SIGMOID = 1 };

const char *nsr_status_string(int status);
/* ABI version; bumped on any signature change. */
int nsr_abi_version(void);
/* "gfx950" -- the only code object in the library. */
const char *nsr_target_arch(void);

/* ------------------------------------------------------------------------------------------
 * _raymarching replacements
 * ------------------------------------------------------------------------------------------ */

/* replaces near_far_from_aabb (raymarching.h:6, raymarching.cu:190-255).
 * rays_o, rays_d [N,3] f32; aabb [6] f32 (device); nears, fars [N] f32. */
int nsr_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N,
                           float min_near, float *nears, float *fars, nsr_stream_t stream);

/* replaces morton3D (raymarching.h:8, raymarching.cu:313-331). coords [N,3] i32 -> indices [N] i32 */
int nsr_morton3d(const int32_t *coords, uint32_t N, int32_t *indices, nsr_stream_t stream);

/* replaces morton3D_invert (raymarching.h:9, raymarching.cu:336-359). */
int nsr_morton3d_invert(const int32_t *indices, uint32_t N, int32_t *coords, nsr_stream_t stream);

/* replaces packbits (raymarching.h:10, raymarching.cu:366-399).
 * grid f32 [N*8]; bitfield u8 [N]; bit i of byte n = grid[8n+i] > density_thresh. */
int nsr_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield,
                 nsr_stream_t stream);

/* replaces march_rays_train (raymarching.h:12, raymarching.cu:410-599).
 *
 * Same outputs as the reference kernel, with one strengthening: sample offsets come from an
 * exclusive scan over ray index instead of atomicAdd arrival order (raymarching.cu:506-507),
 * so `rays` is deterministic: row n = (n, offset_n, count_n).  That is one of the orders the
 * reference can produce.  counter[0] += total samples, counter[1] += N (the reference's
 * atomics), so a non-zero incoming counter offsets the allocation exactly as there.
 *
 * xyzs [M,3], deltas [M,4] f32 (slots 2,3 only written when is_ndc), dirs [M,3] or NULL (the
 * model on this path is built with use_dir=False and never reads it), rays [N,3] i32,
 * counter [2] i32, noises [N] f32 or NULL (= zeros: perturb is force-disabled,
 * raymarching.py:247), z_hats [N] or NULL when !is_ndc.
 * Rays with offset+count >= M are dropped like the reference does (raymarching.cu:517).
 * grid: the bitfield of C cascades of H^3 cells, C * H^3 / 8 bytes.  H must be a power of two in 8..512 (a Morton index is
 * below H^3 only then: any other H would be read past the bitfield) and C <= 8; anything else -> NSR_ERR_INVALID_ARG.
 * workspace: nsr_march_rays_train_workspace_bytes(N, bound, max_steps) bytes of device scratch (per-ray counts, block sums
 * and, for batches marched one thread per ray, a bit mask of bound * max_steps step indices per ray: the counting pass marks
 * the samples, the emitting pass replays the t sequence without probing the grid again; batches marched one wave per ray
 * record the start and the 64-bit sample mask of every 64-step block instead, and their emit replays those). */
uint64_t nsr_march_rays_train_workspace_bytes(uint32_t N, float bound, uint32_t max_steps);
int nsr_march_rays_train(const float *rays_o, const float *rays_d, const float *z_hats,
                         const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps,
                         int is_ndc, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                         const float *nears, const float *fars, float *xyzs, float *dirs,
                         float *deltas, int32_t *rays, int32_t *counter, const float *noises,
                         void *workspace, nsr_stream_t stream);

/* replaces composite_rays_train_forward (raymarching.h:14, raymarching.cu:806-890).
 * sigmas [M], rgbs [M,C], deltas [M,4], rays [N,3] -> weights_sum [N], depth [N], image [N,C].
 * M is the sample-buffer size the march used for its "offset+count >= M" drop test
 * (raymarching.cu:517,830): pass the same value.  C <= 16. */
int nsr_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                     const int32_t *rays, uint32_t M, uint32_t N,
                                     uint32_t C, float T_thresh, int is_ndc, float *weights_sum,
                                     float *depth, float *image, nsr_stream_t stream);

/* replaces composite_rays_train_backward (raymarching.h:15, raymarching.cu:904-997).
 * The reference needs grad_sigmas, grad_rgbs pre-zeroed and an [N,C] scratch rgbs_buf
 * (raymarching.py:339-341); here the running colour sum lives in registers, rgbs_buf is gone,
 * and every sample that belongs to a ray (early-stopped tails and dropped rays included) gets its
 * gradient written -- zeros where the reference leaves the pre-filled zero -- so the buffers need
 * NOT arrive zeroed; only padding samples that belong to no ray are left untouched. */
int nsr_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image,
                                      const float *sigmas, const float *rgbs, const float *deltas,
                                      const int32_t *rays, int is_ndc, const float *weights_sum,
                                      const float *image, uint32_t M, uint32_t N,
                                      uint32_t C, float T_thresh, float *grad_sigmas, float *grad_rgbs,
                                      nsr_stream_t stream);

/* Training composite + the epilogue of Renderer.render_train (renderer.py:225-233) in one launch (no reference
 * counterpart: the reference runs composite_rays_train, then torch ops for `image + (1 - weights_sum)`, the class slice
 * and `clamp(depth - nears, 0) / (fars - nears)`).  Same arithmetic as nsr_composite_rays_train_forward; additionally
 * writes rgb_map [N,3] = image[:, :3] + (1 - weights_sum), classes [N, C-3] = image[:, 3:] (NULL allowed when C == 3) and
 * depth_norm [N].  weights_sum, depth (raw) and image [N,C] are still written (the backward reads weights_sum / image). */
int nsr_render_train_forward(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays,
                             const float *nears, const float *fars, uint32_t M, uint32_t N, uint32_t C, float T_thresh,
                             float *weights_sum, float *depth, float *image, float *rgb_map, float *depth_norm,
                             float *classes, nsr_stream_t stream);
/* Backward of nsr_render_train_forward with respect to sigmas / rgbs, from the gradients of rgb_map [N,3], classes
 * [N, C-3] and weights_sum [N] (each may be NULL = zero; depth_norm carries no gradient, as in the reference whose
 * composite backward ignores grad_depth, raymarching.py:333).  Every sample of every ray gets its gradient written. */
int nsr_render_train_backward(const float *grad_rgb_map, const float *grad_classes, const float *grad_weights_sum,
                              const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays,
                              const float *weights_sum, const float *image, uint32_t M, uint32_t N, uint32_t C,
                              float T_thresh, float *grad_sigmas, float *grad_rgbs, nsr_stream_t stream);

/* Per-ray geometry terms on the weights of the training composite (no reference counterpart: its composite backward drops
 * grad_depth and the weights never leave its kernels).  Samples, columns (is_ndc), live rule and the "offset + steps < M"
 * drop test are nsr_composite_rays_train_forward's; w_i its weights, t_i the running sum of deltas[:, col + 1],
 * delta_i = deltas[:, col], R = fars[index] - nears[index]:
 *   depth [N]      = max(sum_i w_i t_i - near, 0) / R            (what nsr_render_train_forward writes as depth_norm)
 *   distortion [N] = (sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 delta_i) / R       (mip-NeRF 360, eq. 15)
 * Both are 0 for a dropped ray, a ray without samples and a ray whose R is not a positive finite number (a ray that misses
 * the box has near == far == FLT_MAX), where depth_norm is 0 / 0.
 * totals: caller-allocated [N,4] f32 (16 B per ray), written by the forward and read by the backward.  deltas 8-byte aligned.
 * No atomics, no host read, capture-safe; two calls give the same bits. */
int nsr_ray_geometry_forward(const float *sigmas, const float *deltas, const int32_t *rays, const float *nears,
                             const float *fars, uint32_t M, uint32_t N, float T_thresh, int is_ndc, float *depth,
                             float *distortion, float *totals, nsr_stream_t stream);
/* d/d sigmas of nsr_ray_geometry_forward from grad_depth [N] and grad_distortion [N] (each may be NULL = zero), with the
 * live set held constant and exact on every live sample, the one the ray stops on included.  grad_sigmas [M] is WRITTEN
 * (not accumulated) for every sample that belongs to a ray -- zeros behind the stop, for dropped rays and for rays without a
 * range -- and left untouched elsewhere, so it need not arrive zeroed. */
int nsr_ray_geometry_backward(const float *grad_depth, const float *grad_distortion, const float *sigmas,
                              const float *deltas, const int32_t *rays, const float *nears, const float *fars,
                              const float *totals, uint32_t M, uint32_t N, float T_thresh, int is_ndc, float *grad_sigmas,
                              nsr_stream_t stream);

/* Position gradients of the marched samples back to their rays (no reference counterpart), for xyz_i = o + t_i d with the
 * t_i, the samples and their count held constant:  grad_rays_o [N,3] = sum_i g_i,  grad_rays_d [N,3] = sum_i t_i g_i over the
 * ray's samples, g = grad_xyzs [M,3].  The walk, the running parameter (sum scan of deltas[:, 1] carried across trips) and the
 * "offset + steps < M" drop test are nsr_composite_rays_train_forward's; pass the march's M.
 * nears [N] or NULL.  The march emits deltas[:, 1] = t_next - last_t with last_t starting at the ray's first parameter
 * (nears[index] when noises == NULL), so the running sum is the parameter behind the sample, measured from that start: with
 * nears the sample's own parameter t_i = nears[index] + sum_{j<=i} deltas[j, 1] - deltas[i, 0] is used -- where the march put
 * xyz_i; with NULL the running sum itself.  Rows are indexed by rays[:, 0]; dropped rays and rays without samples get zeros.
 * deltas 8-byte aligned.  No atomics, no host read, capture-safe; two calls give the same bits.
 * is_ndc != 0 -> NSR_ERR_UNSUPPORTED (an NDC sample is not o + t d of the rays the march was given). */
int nsr_rays_position_backward(const float *grad_xyzs, const float *deltas, const int32_t *rays, const float *nears,
                               uint32_t M, uint32_t N, int is_ndc, float *grad_rays_o, float *grad_rays_d,
                               nsr_stream_t stream);

/* Reconstruction loss of Trainer.calc_loss (trainers/base.py:251-304), value AND gradient in one pass:
 *   loss = mean((rgb_map - target_rgb[pix])^2) + ce_lambda * mean(logsumexp(classes) - classes[target_cls[pix]])
 * (nn.MSELoss + 0.001 * nn.CrossEntropyLoss on the class logits; the reference builds it from ~25 torch kernels and as
 * many again in autograd).  pix [N] int64 = rows of the targets (NULL: row n); target_rgb [P,3] f32; target_cls [P] int64.
 * classes == NULL, nc == 0 or ce_lambda == 0: MSE only (grad_classes untouched).
 * Everything is multiplied by factor * (scale ? scale[0] : 1): `scale` is the device-side loss scale (nsr_scaler_update),
 * `factor` e.g. 1 / world size.  loss_out [3] = {scaled total, unscaled mse, unscaled ce_lambda * ce}.  The value is summed in
 * a fixed order (block tree + one-block final pass): run-to-run identical.
 * workspace: nsr_recon_loss_workspace_bytes(N) bytes. */
uint64_t nsr_recon_loss_workspace_bytes(uint32_t N);
int nsr_recon_loss(const float *rgb_map, const float *classes, uint32_t N, uint32_t nc, const float *target_rgb,
                   const int64_t *target_cls, const int64_t *pix, float ce_lambda, float factor, const float *scale,
                   float *grad_rgb_map, float *grad_classes, float *loss_out, void *workspace, nsr_stream_t stream);

/* nsr_recon_loss with a weight per ray (importance sampling, nsr_draw_frame_batch_error below):
 *   loss = (1/3N) sum_n w_n |rgb_map_n - target_n|^2 + ce_lambda * (1/N) sum_n w_n (logsumexp(classes_n) - classes_n[label_n])
 * ray_weight [N] f32 (NULL: every weight 1) multiplies every per-ray term of the value and of both gradients; the means still
 * divide by N.  ray_err [N] f32 (optional) receives the ray's UNWEIGHTED sum over the three channels of (rgb_map - target)^2
 * (the fp32 differences, their squares summed in fp64 and rounded once), what nsr_error_map_accumulate takes.  Same grid, block tree, final pass, loss_out and workspace
 * (nsr_recon_loss_workspace_bytes) as nsr_recon_loss; with every weight exactly 1.0f the value and the gradients are
 * bit-identical to nsr_recon_loss's. */
int nsr_recon_loss_weighted(const float *rgb_map, const float *classes, uint32_t N, uint32_t nc, const float *target_rgb,
                            const int64_t *target_cls, const int64_t *pix, const float *ray_weight, float ce_lambda, float factor,
                            const float *scale, float *grad_rgb_map, float *grad_classes, float *ray_err, float *loss_out,
                            void *workspace, nsr_stream_t stream);

/* nsr_recon_loss_weighted with a gain per frame and colour channel (per-frame exposure and white balance of a mixed-frame batch).
 * exposure [F,3] f32: log2 gains, zero is identity.  The batch is S segments of K rays (N == S * K), ray n belongs to segment
 * s = n / K and frame f = seg_frame[s] (seg_frame [S] i32, nsr_draw_frame_batch).  With w = ray_weight[n] (NULL: 1),
 * s_ = scale * factor, inv3n = 1 / (3N), row = pix[n] (NULL: n), per ray and channel c in fp32:
 *   gain = 0 <= f < F ? exp2f(exposure[f,c]) : 1          a frame outside [0, F) reads no exposure row
 *   p    = rgb_map[n,c] * gain                            what frame f is modelled to have observed (a product rounded on its own)
 *   df   = p - target_rgb[row,c]
 *   mse += (w * df) * df                                  the MSE term of loss_out, as in nsr_recon_loss_weighted
 *   gp   = 2 * df * inv3n * s_ * w                        d loss / d p
 *   grad_rgb_map[n,c] = gp * gain
 *   ray_err[n] (optional) = sum_c (f64)df * (f64)df, rounded once: the exposure-corrected error
 *   term[n,c] = gp * p                                    fp32, staged in the workspace
 *   grad_exposure[f,c] = (f32)(ln2 * sum over the rays n of frame f of (f64)term[n,c])
 * The cross-entropy term, grad_classes, loss_out[0..2], the grid, the block tree and the final pass are nsr_recon_loss_weighted's.
 * grad_exposure [F,3] f32 is WRITTEN for every frame and carries scale * factor as grad_rgb_map does; a frame that no segment
 * names gets +0.0, a segment whose frame is outside [0, F) contributes to no row.
 * Order of the per-frame sum (fp64 throughout, rounded to fp32 once; no atomics, no counters; two calls and the replays of a
 * captured graph give the same bits), that of nsr_generate_rays_frames_backward:
 *   per segment, K < 64:  one thread adds the segment's rays in ascending n.
 *   per segment, K >= 64: B = min(ceil(K / 256), 64) blocks of 256 threads; thread t of block b adds rays k = b * 256 + t,
 *                         k += B * 256, of the segment in that order; a wave adds its 64 lanes by a butterfly (lane ^ 32, 16, 8,
 *                         4, 2, 1), the block its four waves in ascending order; then the B block sums in ascending b.
 *   per frame:            the sums of the segments naming it, in ascending s.
 * With exposure all zero, loss_out, grad_rgb_map, grad_classes and ray_err are bit-identical to nsr_recon_loss_weighted's.
 * workspace: nsr_recon_loss_exposure_workspace_bytes(N, F, S, K) bytes, 8-byte aligned; nothing of it is read that this call did
 * not write.  N == 0, F == 0, S == 0, K == 0 or N != S * K -> NSR_ERR_INVALID_ARG before any pointer is looked at; the other
 * checks are nsr_recon_loss's, and exposure, seg_frame and grad_exposure must not be NULL. */
uint64_t nsr_recon_loss_exposure_workspace_bytes(uint32_t N, uint32_t F, uint32_t S, uint32_t K);
int nsr_recon_loss_exposure(const float *rgb_map, const float *classes, uint32_t N, uint32_t nc, const float *target_rgb,
                            const int64_t *target_cls, const int64_t *pix, const float *ray_weight, const float *exposure, uint32_t F,
                            const int32_t *seg_frame, uint32_t S, uint32_t K, float ce_lambda, float factor, const float *scale,
                            float *grad_rgb_map, float *grad_classes, float *grad_exposure, float *ray_err, float *loss_out,
                            void *workspace, nsr_stream_t stream);

/* Matting-Laplacian photorealism loss of Deep Photo Style Transfer, the reference's MattingLaplacian (loss.py:217-278,
 * win_rad r, eps): loss_out[0] (device fp64) = trace(V M V^T), M the matting Laplacian of `target` over every (2r+1)^2
 * window inside the image, V = v reshaped [3, H*W]; grad_v (may be NULL) [3,H,W] f32 = d loss / d v, rounded once.
 * Matrix-free (no HW x HW matrix): inputs are read in f32 and every operation is fp64.  target, v [3,H,W] f32.
 * r in {1, 2} (else NSR_ERR_UNSUPPORTED); H, W >= 2r+1.  No atomics: the value is summed in a fixed order (block partials +
 * one-block final pass), so value and gradient are run-to-run identical.
 * workspace: nsr_matting_laplacian_workspace_bytes(H, W, win_rad) bytes, 8-byte aligned. */
uint64_t nsr_matting_laplacian_workspace_bytes(uint32_t H, uint32_t W, uint32_t win_rad);
int nsr_matting_laplacian(const float *target, const float *v, uint32_t H, uint32_t W, uint32_t win_rad, double eps,
                          double *loss_out, float *grad_v, void *workspace, nsr_stream_t stream);

/* Colour transfer of pixel rows to a style image (ARF's colour matching, the reference's match_colors_for_image_set,
 * utils/__init__.py:262-295): the two passes over the rows; the 3x3 eigen-solve between them is host code
 * (nerfstyle_amd/color_match.py).  rows / src / dst: n rows of `stride` f32, stride 3 (R, G, B) or 4 (R, G, B and one float
 * that is never read as colour); 4-byte aligned, 16-byte aligned for stride 4.
 *
 * nsr_color_moments: moments [9] (device fp64, 8-byte aligned) = sum r, sum g, sum b, sum rr, sum rg, sum rb, sum gg, sum gb,
 * sum bb over the n rows.  Every value is converted to fp64 first (the products are then exact) and every sum is fp64.
 * Order of summation, a function of n and stride only (no atomics, nothing depends on the device or on timing; two calls give
 * the same 72 bytes):
 *   unit:    stride 4: one row, U = n units.  stride 3: four consecutive rows 4u .. 4u+3 (the last unit may hold fewer), added
 *            in ascending order, U = ceil(n / 4) units.
 *   grid:    B = clamp(ceil(U / 1024), 1, 2048) blocks of 256 threads, T = 256 B.
 *   thread:  thread t of the grid adds units t, t + T, t + 2T, ... in that order into nine accumulators that start at +0.
 *   wave:    butterfly over the 64 lanes (lane ^ 32, 16, 8, 4, 2, 1).
 *   block:   its four wave sums in ascending order, starting from +0 -> partial[b] in the workspace.
 *   final:   one block of 256 threads; thread t adds partial[t], partial[t + 256], ... in that order, then wave and block as above.
 * workspace: nsr_color_moments_workspace_bytes(n) bytes (enough for either stride), 8-byte aligned; nothing of it is read that
 * this call did not write.  n == 0, stride outside {3, 4}, a NULL or misaligned pointer -> NSR_ERR_INVALID_ARG, nothing written.
 *
 * nsr_color_apply: with tf [4,4] f32 row-major in DEVICE memory (read by the kernel: a captured graph sees what was last written
 * there; its last row is not read), per row and c in 0..2, in f32:
 *   dst[i,c] = fmaf(tf[c,2], b, fmaf(tf[c,1], g, fmaf(tf[c,0], r, tf[c,3])))        (r, g, b) = src[i,0..2]
 *   clamp != 0:  dst[i,c] = fminf(fmaxf(dst[i,c], 0), 1)
 * stride 4: dst[i,3] = src[i,3] bit for bit.  dst == src (in place) is allowed; src and dst that overlap otherwise are refused.
 * n == 0, stride outside {3, 4}, a NULL or misaligned pointer, such an overlap -> NSR_ERR_INVALID_ARG, nothing written.
 * Neither call reads the host or allocates; both are capture-safe. */
uint64_t nsr_color_moments_workspace_bytes(uint64_t n);
int nsr_color_moments(const float *rows, uint64_t n, uint32_t stride, double *moments, void *workspace, nsr_stream_t stream);
int nsr_color_apply(const float *src, float *dst, uint64_t n, uint32_t stride, const float *tf, int clamp, nsr_stream_t stream);

/* Region-wise colour transfer: the same two passes with one set of moments and one transform per region (a scene class on the
 * content side, a style cluster on the style side; nerfstyle_amd/color_match.py solves one 3x3 pair per matched region on the
 * host).  rows / src / dst and their alignment as above.  K regions, 1 <= K <= NSR_COLOR_MAX_REGIONS, and slot K for every
 * row that belongs to none of them.
 *
 * region(i):  labels != NULL (i32 [n], 4-byte aligned): labels[i] when 0 <= labels[i] < K, else K.
 *             labels == NULL (stride 4 only): with w the row's fourth float, k when w == (float)k for an integer 0 <= k < K
 *             (-0.0 is 0), else K: negative, >= K, fractional, NaN and inf all select slot K.
 * The fourth float of a stride-4 row is a label or ignored, never a colour; nsr_color_region_apply carries it bit for bit.
 *
 * nsr_color_region_moments: moments [K+1][10] (device fp64, 8-byte aligned); moments[k] = count, sum r, sum g, sum b, sum rr,
 * sum rg, sum rb, sum gg, sum gb, sum bb over the rows of region k, values converted to fp64 first, every sum fp64, the count
 * exact.  A region without rows is ten +0.0.  No floating-point atomics anywhere.  Order of summation, a function of
 * (n, stride, K, region(.)) only -- not of the alignment of rows or labels, which decides the loads alone:
 *   unit, grid: those of nsr_color_moments (U units, B blocks of 256 threads, T = 256 B), so a wave of 64 lanes holds 64
 *            consecutive units per trip; wave w of the grid takes units 64 w + lane + j T, j = 0, 1, ... in that order.
 *   slot:    stride 4: the lane's row.  stride 3: rows 4u, 4u+1, 4u+2, 4u+3 of the lane's unit, one slot after the other.
 *   region:  per slot, while lanes remain: k = region of the lowest remaining lane; the lanes of region k contribute their nine
 *            values, all others +0.0, to the butterfly over the 64 lanes (lane ^ 32, 16, 8, 4, 2, 1); the nine sums and the
 *            number of those lanes (as a double) are added to entry k of the wave's own table; those lanes are done.
 *   block:   entry by entry its four waves' tables in ascending order, starting from +0 -> partial[b][K+1][10] in the workspace.
 *   final:   one block of 256 threads per region; thread t adds partial[t][k], partial[t + 256][k], ... in that order, then
 *            butterfly and the four wave sums in ascending order from +0.
 * workspace: nsr_color_region_moments_workspace_bytes(n, K) bytes (enough for either stride; 0 for K outside 1..64), 8-byte
 * aligned; nothing of it is read that this call did not write.
 *
 * nsr_color_region_apply: tfs [K+1][4][4] f32 row-major in DEVICE memory (read by the kernel; the last row of each is not
 * read); row i is mapped by tfs[region(i)] with exactly the fma chain and clamp of nsr_color_apply: with all K+1 transforms
 * equal the output is that of nsr_color_apply bit for bit.  dst == src is allowed, src and dst that overlap otherwise are refused.
 *
 * Both: n == 0, stride outside {3, 4}, K == 0 or K > NSR_COLOR_MAX_REGIONS, labels == NULL with stride 3, a NULL or misaligned
 * pointer, such an overlap -> NSR_ERR_INVALID_ARG, nothing launched.  Neither call reads the host, allocates or synchronises;
 * both are capture-safe. */
#define NSR_COLOR_MAX_REGIONS 64
uint64_t nsr_color_region_moments_workspace_bytes(uint64_t n, uint32_t K);
int nsr_color_region_moments(const float *rows, uint64_t n, uint32_t stride, const int32_t *labels, uint32_t K, double *moments,
                             void *workspace, nsr_stream_t stream);
int nsr_color_region_apply(const float *src, float *dst, uint64_t n, uint32_t stride, const int32_t *labels, uint32_t K,
                           const float *tfs, int clamp, nsr_stream_t stream);

/* replaces march_rays (raymarching.h:17, raymarching.cu:1004-1130), inference.  noises [n_alive] f32 or NULL (= zeros).
 * C, H as for nsr_march_rays_train: H a power of two in 8..512, C <= 8, else NSR_ERR_INVALID_ARG. */
int nsr_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t,
                   const float *rays_o, const float *rays_d, const float *z_hats, float bound,
                   float dt_gamma, uint32_t max_steps, int is_ndc, uint32_t C, uint32_t H,
                   const uint8_t *grid, const float *nears, const float *fars, float *xyzs, float *dirs,
                   float *deltas, const float *noises, nsr_stream_t stream);

/* replaces composite_rays (raymarching.h:18, raymarching.cu:1133-1240), inference, in place. */
int nsr_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive,
                       float *rays_t, const float *sigmas, const float *rgbs, const float *deltas,
                       uint32_t C, int is_ndc, float *weights_sum, float *depth, float *image,
                       nsr_stream_t stream);

/* Single-pass inference composite (no reference counterpart as one call): kernel_composite_rays'
 * arithmetic (raymarching.cu:1133-1231: T = 1 - weight_sum, stop test before the sample, absolute t
 * from nears[ray]) over the compacted samples [offset, offset+count) that nsr_march_rays_train
 * emits -- replaces the host loop of up to max_steps march_rays / composite_rays iterations
 * (renderer.py:266-285).  Outputs are written (not accumulated). */
int nsr_composite_rays_infer(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays,
                             const float *nears, uint32_t M, uint32_t N, uint32_t C, float T_thresh,
                             float *weights_sum, float *depth, float *image, nsr_stream_t stream);

/* Alive-ray compaction on the device (replaces the boolean-mask `rays_alive[rays_alive >= 0]`
 * of renderer.py:284, which is a host sync): stable, ballot/scan based.
 * out [n_alive] i32, n_out [1] i32 (device).  workspace: nsr_compact_alive_workspace_bytes(n). */
uint64_t nsr_compact_alive_workspace_bytes(uint32_t n_alive);
int nsr_compact_alive(const int32_t *rays_alive, uint32_t n_alive, int32_t *out, int32_t *n_out,
                      void *workspace, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * _gridencoder replacements
 * ------------------------------------------------------------------------------------------ */

/* gridencoder.cu:137 evaluated once on the host: resolution[l] = floor(exp2f(l*S)*H), fp32.
 * The kernels take this table instead of re-evaluating exp2f per thread. res_out host [L]. */
int nsr_grid_resolutions(uint32_t L, float S, uint32_t H, uint32_t *res_out);

/* replaces grid_encode_forward (gridencoder.h:12, gridencoder.cu:83-235,439-461), D = 3.
 * inputs [B,3] f32 in [0,1]; embeddings [rows,C] of emb_dtype (NSR_F32|NSR_F16);
 * offsets HOST [L+1] i32 (the reference passes a device tensor; it is 17 ints);
 * outputs of emb_dtype: layout [L,B,C] when out_blc == 0 (the reference kernel's) or
 * [B,L*C] when out_blc != 0 (what grid.py:58 returns after its permute+reshape copy).
 * Rows whose input is outside [0,1] (gridencoder.cu:107-132) or NaN are written as zeros.
 * calc_grad_inputs != 0 -> NSR_ERR_UNSUPPORTED: no dy_dx buffer is written here; the input gradient comes from
 * nsr_grid_encode_input_backward, which recomputes the partials.
 * C in {1,2,4,8} like the reference; L <= 32. */
int nsr_grid_encode_forward(const float *inputs, const void *embeddings, int emb_dtype,
                            const int32_t *offsets, void *outputs, uint32_t B, uint32_t D, uint32_t C,
                            uint32_t L, float S, uint32_t H, int calc_grad_inputs, uint32_t gridtype,
                            int align_corners, uint32_t style, int out_blc, nsr_stream_t stream);

/* replaces grid_encode_backward (gridencoder.h:13, gridencoder.cu:238-328,464-494).
 * grad of grad_dtype in the layout selected by grad_blc; grad_embeddings [rows,C] f32 ALWAYS
 * (fp32 atomics; the reference accumulates in half under AMP) and arrives zeroed or holding a
 * running sum (the kernel accumulates).  Rows whose input is outside [0,1] or NaN add nothing. */
int nsr_grid_encode_backward(const void *grad, int grad_dtype, const float *inputs,
                             const int32_t *offsets, float *grad_embeddings, uint32_t B, uint32_t D,
                             uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                             int align_corners, uint32_t style, int grad_blc, nsr_stream_t stream);

/* replaces the calc_grad_inputs half of the reference (dy_dx of gridencoder.cu:189-234 + kernel_input_backward :331-357)
 * without a dy_dx [B, L*D*C] buffer: one thread per sample recomputes the partials from the table and writes
 * grad_inputs [B,3] f32 = sum over levels (ascending) and channels of grad * d output / d input.  No atomics: two calls give
 * the same bits.  grad of grad_dtype (NSR_F32|NSR_F16) in the layout grad_blc selects, embeddings of emb_dtype
 * (NSR_F32|NSR_F16), offsets HOST [L+1]; rows whose input is outside [0,1] (gridencoder.cu:121-130) or NaN get zeros.
 * D != 3 -> NSR_ERR_UNSUPPORTED; C in {1,2,4,8}; L <= 32. */
int nsr_grid_encode_input_backward(const void *grad, int grad_dtype, const float *inputs, const void *embeddings,
                                   int emb_dtype, const int32_t *offsets, float *grad_inputs, uint32_t B, uint32_t D,
                                   uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                   uint32_t style, int grad_blc, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * tcnn.Network replacement: bias-free fully fused MLP on MFMA
 * ------------------------------------------------------------------------------------------
 * params: fp32 master weights, flat, row-major [out,in] per layer, layers concatenated, the
 * last layer's rows padded to a multiple of 16 (nsr_mlp_param_count).  Hidden width 64, ReLU.
 * Compute contract: inputs, weights and hidden activations rounded to compute_dtype
 * (NSR_F16 | NSR_BF16), products accumulated in fp32 by v_mfma_f32_16x16x32_{f16,bf16} (K = 32 layers) and the
 * 16x16x16 forms (a 16-wide first layer, the output layer's transpose in the backward, every weight gradient).
 * x [M,n_in] f32, 16-byte aligned; y [M,n_out] f32 (after out_act).  n_in in {16,32}; 1 <= n_out <= 16;
 * n_hidden_layers in {1,2}; n_neurons == 64; anything else -> NSR_ERR_UNSUPPORTED.  An out_act other than
 * NSR_ACT_NONE | NSR_ACT_SIGMOID, or x off 16-byte alignment -> NSR_ERR_INVALID_ARG.  M == 0 -> NSR_OK.  Nothing is
 * written on an error. */
uint32_t nsr_mlp_param_count(uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers);
int nsr_mlp_forward(const float *x, const float *params, uint32_t M, uint32_t n_in, uint32_t n_out,
                    uint32_t n_neurons, uint32_t n_hidden_layers, int out_act, int compute_dtype,
                    float *y, nsr_stream_t stream);
/* dy [M,n_out] f32 = dL/dy (post-activation); y [M,n_out] the forward output (for sigmoid').
 * dx [M,n_in] f32 (16-byte aligned) or NULL; dparams [count] f32 or NULL is ACCUMULATED into (fp32 atomics, one add per
 * workgroup per non-zero weight gradient).  Activations are recomputed, nothing is saved by the forward: y may be NULL. */
int nsr_mlp_backward(const float *x, const float *params, const float *y, const float *dy, uint32_t M,
                     uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers,
                     int out_act, int compute_dtype, float *dx, float *dparams, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused field: BBox.normalize -> 2x hash encode -> 4 MLPs -> trunc_exp / sigmoid / cat
 * (networks/style_nerf.py:120-142, use_dir = False) in ONE launch per direction.
 * ------------------------------------------------------------------------------------------
 * Data layout (MI355X-first): the two hash tables are stored INTERLEAVED,
 *   tables[row][enc][feat], enc 0 = x_density_embedder, enc 1 = x_color_embedder, feat < 2,
 * so that one 16-byte (f32) / 8-byte (f16) load or one 64-byte atomic request serves both
 * encoders (same positions, same hash => same row).  grad_tables has the same layout, f32.
 * mlp_params: the four flat fp32 parameter vectors concatenated in the order
 *   density (32->64->1), color1 (32->64->16), color2 (16->64->64->3), class (32->64->nc);
 * grad_mlp likewise (accumulated into).
 */
typedef struct nsr_field_desc {
    uint32_t L;                /* levels (16) */
    uint32_t H;                /* base resolution (16) */
    float S;                   /* log2(per_level_scale), fp32 (grid.py:36) */
    uint32_t num_classes;      /* nc <= 13; output channels C_ch = 3 + nc */
    int table_dtype;           /* NSR_F32 | NSR_F16: element type of `tables` */
    int compute_dtype;         /* NSR_F16 | NSR_BF16 for the MFMA chain */
    float bbox_min[3];         /* BBox.normalize: x_hat = (x - min) / size (common.py:276-288) */
    float bbox_size[3];
    float density_scale;       /* renderer.py:225, folded into sigma */
    const int32_t *offsets;    /* HOST [L+1], rows (grid.py:129-140) */
} nsr_field_desc;

/* xyzs [M,3] f32 world positions.  sigmas [M] f32 = exp(logit) * density_scale;
 * rgbs [M, 3+nc] f32 = cat(sigmoid(rgb), classes) or NULL for the sigma-only branch
 * (style_nerf.py:125-126).  m_dev: optional device int32 sample count (<= M) -- tiles past it
 * are skipped, so callers can size M as a capacity and never read the count on the host.
 * feats (optional, may be NULL): ceil(M/16)*2048 bytes that receive the encoded features of both
 * encoders as ready-made MFMA B fragments (128 B per sample, the only thing a training forward
 * saves); pass the same buffer to nsr_field_backward to skip its re-gather. */
/* perm (optional, may be NULL): device uint32 [M] from nsr_sample_order -- the kernel's tile t then works on samples
 * perm[16t .. 16t+15] of the buffers (outputs land at those samples' own slots; `feats` stays tile-major, so the
 * backward must be given the same perm).  Results per sample are bit-identical with and without it. */
int nsr_field_forward(const nsr_field_desc *desc, const void *tables, const float *mlp_params,
                      const float *xyzs, uint32_t M, const int32_t *m_dev, float *sigmas, float *rgbs,
                      void *feats, const uint32_t *perm, nsr_stream_t stream);

/* Density and its gradient with respect to the world position, forward mode, one launch (csrc/field_normal.hip): the
 * density encoder's features and their three spatial tangents go through the density net together; nothing is saved, no
 * atomics.  Reads the density half of `tables` only.  sigmas [M] f32 or NULL: bit-identical to nsr_field_forward with
 * rgbs == NULL.  grads [M,3] f32 = density_scale * exp(clamp(logit,-15,15)) * d logit / d x (the trunc_exp rule of the
 * backward); with normalize != 0 the unit normal -grad / |grad| instead, for every gradient with finite components (a zero
 * gradient stays a zero vector).
 * Samples whose position is NaN or encodes outside [0,1] get the forward's sigma and a zero gradient; slots at or past
 * *m_dev keep their sigma and get a zero gradient.  Capture-safe, no host read.  L != 16 -> NSR_ERR_UNSUPPORTED. */
int nsr_field_density_gradient(const nsr_field_desc *desc, const void *tables, const float *mlp_params,
                               const float *xyzs, uint32_t M, const int32_t *m_dev, float *sigmas, float *grads,
                               int normalize, nsr_stream_t stream);

/* grad_sigmas [M], grad_rgbs [M,3+nc] f32.  Recomputes the forward (nothing saved), then
 * back-propagates: trunc_exp' = exp(clamp(logit,-15,15)) (tcnn_nerf.py:62-66), sigmoid', ReLU
 * masks, MLP dgrad on MFMA, wgrad on MFMA (accumulated into grad_mlp), and scatters the
 * encoder gradient into grad_tables with fp32 atomics (both encoders per request).
 * train_density_table / train_color_table: 0 skips that encoder's scatter (stylisation
 * optimises x_color_embedder only, trainers/style.py:25).  grad_mlp may be NULL: no weight gradient is produced; with perm,
 * saved feats, train_density_table = 0 and grad_mlp = NULL (exactly the stylisation stage) a colour-only kernel runs that
 * computes the class / colour nets' input gradients and nothing else. */
int nsr_field_backward(const nsr_field_desc *desc, const void *tables, const float *mlp_params,
                       const float *xyzs, uint32_t M, const int32_t *m_dev, const float *grad_sigmas,
                       const float *grad_rgbs, float *grad_tables, float *grad_mlp,
                       int train_density_table, int train_color_table, const void *feats,
                       const uint32_t *perm, void *workspace, nsr_stream_t stream);
/* feats given together with perm must come from nsr_field_forward called with the SAME perm (they are tile-major in
 * perm's order; the first kernel below walks that order).
 * perm != NULL (nsr_sample_order): the MLP backward writes every sample's encoder-output gradient (256 B) to
 * `workspace` and a second, high-occupancy kernel accumulates the table gradient walking the samples in perm's
 * spatial order (LDS lattices, one merged atomic record per touched corner; csrc/table_scatter.hip).  Pays on dense
 * (full-frame) batches; results equal the perm == NULL call up to fp32 summation order.
 * workspace: nsr_field_backward_workspace_bytes(M, with_perm) bytes, 16-byte aligned (0 / NULL without perm). */
uint64_t nsr_field_backward_workspace_bytes(uint32_t M, int with_perm);
/* Contract of the workspace after nsr_field_backward / _dirs with perm != NULL: its first M * 256 bytes are
 * enc_grad [M][16] float4, sample-major: entry [m][l] = d loss / d (density feature 0, density feature 1, colour feature 0,
 * colour feature 1) of level l of the sample in slot m (its own slot, whatever perm's order), for every slot below the count.
 * Slots at or past *m_dev are not written (stale bytes).  The colour-only kernel (perm, saved feats, train_density_table = 0,
 * grad_mlp = NULL: the stylisation stage) writes ZEROS in the density half: the buffer is then not the input of a full
 * position gradient. */

/* d loss / d xyz of every sample from that buffer (csrc/field_xgrad.hip; no reference counterpart): enc_grad contracted with
 * the spatial partials of the trilinear interpolation of both encoders (the arithmetic of nsr_grid_encode_input_backward per
 * level, levels summed in ascending order, fp32) times the derivative of BBox.normalize and the encoder-input map,
 * 1 / (2 * bbox_size[k]).  tables: the interleaved gather tables, f16 or f32 (desc->table_dtype); xyzs [M,3]; perm optional
 * (the samples are then walked in its order; results per sample are bit-identical with and without it).
 * grad_xyzs [M,3] f32 is WRITTEN for every slot: a sample whose position is NaN or encodes outside [0,1], and every slot at
 * or past *m_dev, gets zeros -- the kernel tests that itself and never reads enc_grad there.  enc_grad 16-byte aligned.
 * No atomics, no host read, capture-safe; two calls give the same bits.  L != 16 -> NSR_ERR_UNSUPPORTED. */
int nsr_field_position_gradient(const nsr_field_desc *desc, const void *tables, const float *xyzs, uint32_t M,
                                const int32_t *m_dev, const void *enc_grad, const uint32_t *perm, float *grad_xyzs,
                                nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * View-dependent colour (networks/style_nerf.py with use_dir = True): color2's input is cat(color1 output [16], degree-4
 * spherical harmonics of the viewing direction [16]), its first layer 64 x 32.
 * ------------------------------------------------------------------------------------------
 * The encoding follows tiny-cuda-nn's SphericalHarmonics (the reference feeds (d + 1) / 2, the encoder maps back with
 * 2u - 1 in fp32): 16 coefficients in tiny-cuda-nn's order and sign convention, written down from general knowledge of it --
 * parity with a tiny-cuda-nn build is UNPINNED, like the MLPs'.  Inside the field the coefficients are rounded to the compute
 * type where they enter the MFMA (the MLP contract); nsr_sh_encode returns them in fp32.
 * mlp_params / grad_mlp of the *_dirs entry points hold nsr_field_mlp_param_count(1) = 16384 floats: the 15360 of the plain
 * entry points at the same offsets, then color2's SH columns as a row-major [64,16] block (column j of it is column 16 + j
 * of the reference-shaped first layer).
 * dirs [M,3] f32 follows the sample buffers' conventions: indexed through perm like xyzs, slots at or past *m_dev ignored.
 * Everything else is as in nsr_field_forward / nsr_field_backward; sigmas and the class channels are bit-identical to
 * theirs.  rgbs == NULL (sigma only) never reads dirs. */
uint32_t nsr_field_mlp_param_count(int with_dirs);
/* Host only: 1 when a full (rgbs != NULL) forward of this descriptor with / without perm and directions runs the lattice-gather
 * kernel (16-bit tables, perm given, lattices that fit a quarter of a CU's LDS), 0 when it runs the plain gather kernel. */
int nsr_field_forward_uses_lattice(const nsr_field_desc *desc, int with_perm, int with_dirs);
/* dirs [M,3] f32 -> out [M,16] f32 (16-byte aligned). */
int nsr_sh_encode(const float *dirs, uint32_t M, float *out, nsr_stream_t stream);
int nsr_field_forward_dirs(const nsr_field_desc *desc, const void *tables, const float *mlp_params,
                           const float *xyzs, uint32_t M, const int32_t *m_dev, float *sigmas, float *rgbs,
                           void *feats, const uint32_t *perm, const float *dirs, nsr_stream_t stream);
/* The recomputed forward runs the K = 32 first layer; the SH columns' weight gradient (four more accumulator tiles, skipped
 * with the others when grad_mlp == NULL) lands at grad_mlp + 15360.  No gradient with respect to dirs is produced. */
int nsr_field_backward_dirs(const nsr_field_desc *desc, const void *tables, const float *mlp_params,
                            const float *xyzs, uint32_t M, const int32_t *m_dev, const float *grad_sigmas,
                            const float *grad_rgbs, float *grad_tables, float *grad_mlp,
                            int train_density_table, int train_color_table, const void *feats,
                            const uint32_t *perm, void *workspace, const float *dirs, nsr_stream_t stream);

/* Spatial processing order of marched samples (no reference counterpart; see csrc/sample_order.hip): perm [M] u32 =
 * indices of the first n = min(max(m_dev[0], 0), sort_prefix) samples (m_dev == NULL: n = sort_prefix) in Morton order of
 * their encoder input, stable (ray order inside a 4^3-finest-cell block), followed by the slots n .. M-1 in identity order,
 * whatever their positions hold.  sort_prefix (a larger value is clamped to M) caps the number of leading slots that take part
 * in the sort; the kernels bound themselves by n on the device, so M is the normal value (a smaller one is still correct: the
 * slots past it keep identity order).
 * Key: per axis u = ((x - bbox_min) / bbox_size + 1) / 2, q = floor(clamp(1024 u, 0, 1023)) with NaN -> 0, of which the low 9
 * bits count: q9 = max(q - 512, 0), since u of a position inside the box is in [0.5, 1] and the top bit of its 10-bit
 * coordinate is always set; the key is the 27-bit interleave of the three q9, x in bit 0, y in bit 1, z in bit 2 of every
 * triple.  Positions outside the box sort with its faces (cell 0 or 511 of that axis, -inf and +inf included), NaN as cell 0.
 * The sort is the library's own LSD radix sort (3 x 9 bits): stream-ordered, no host call, capture-safe, deterministic; every
 * counter in the workspace is initialised by the call itself.  Returns before any launch: NSR_OK for M == 0,
 * NSR_ERR_INVALID_ARG for a null xyzs / perm / workspace / box or a workspace that is not 256-byte aligned.
 * Consumed by nsr_field_forward / nsr_field_backward (spatial walk, table scatter in spatial order).
 * workspace: nsr_sample_order_workspace_bytes(M) bytes, 256-byte aligned.  bbox_min / bbox_size: HOST float[3]. */
uint64_t nsr_sample_order_workspace_bytes(uint32_t M);
int nsr_sample_order(const float *xyzs, uint32_t M, const int32_t *m_dev, uint32_t sort_prefix,
                     const float *bbox_min, const float *bbox_size, uint32_t *perm, void *workspace,
                     nsr_stream_t stream);

/* Streaming inference render (renderer.py:237-293 as ONE launch per frame): occupancy march, fused field and the inference
 * composite of nsr_composite_rays_infer in one kernel, with the ray state in registers.  No sample buffer and no capacity:
 * no ray is ever dropped, and a ray that stopped (T < T_thresh) costs nothing further.  Samples, their order and the
 * compositing arithmetic are those of nsr_march_rays_train (noises == NULL) + nsr_field_forward + nsr_composite_rays_infer
 * (raymarching.cu:1133-1231); it is nsr_render_rays_stream below with NSR_STREAM_INFER and no optional output.
 * order: optional device [N] u32, the ray handled k-th (a permutation of 0..N-1; NULL = identity) -- outputs always land in
 * the ray's own row.  weights_sum [N], depth [N], image [N, 3 + desc->num_classes] f32 are written, not accumulated; rays
 * that miss the box (near == far == FLT_MAX) or meet no occupied cell get zeros.  stats: optional device u32[2] that is
 * ACCUMULATED into: {samples shaded, rays finished}.  C, H: cascades and resolution of `grid` (nsr_march_rays_train's; H that
 * is no power of two in 8..512 -> NSR_ERR_INVALID_ARG).
 * No workspace, no host read, capture-safe.  is_ndc != 0, C > 16 or num_classes > 13 -> NSR_ERR_UNSUPPORTED. */
int nsr_render_rays_infer(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *rays_o,
                          const float *rays_d, const uint32_t *order, uint32_t N, const float *nears, const float *fars,
                          const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, int is_ndc, uint32_t C,
                          uint32_t H, float T_thresh, float *weights_sum, float *depth, float *image, uint32_t *stats,
                          nsr_stream_t stream);

/* The streaming render with a choice of composite, and render_train's epilogue in the write-out.  One kernel, no sample
 * buffer, no capacity; the march, the samples and their order are nsr_render_rays_infer's (no NDC).
 *   NSR_STREAM_INFER  composite of nsr_composite_rays_infer (raymarching.cu:1133-1231): T = 1 - weights_sum, the stop test sees T
 *                     in front of the sample, the depth parameter starts at `near`.  With every optional output NULL this IS
 *                     nsr_render_rays_infer.
 *   NSR_STREAM_TRAIN  composite of nsr_composite_rays_train_forward (raymarching.cu:806-879): T is a running product, the ray
 *                     stops when T < T_thresh AFTER a sample, the depth parameter starts at 0.  Equal to nsr_march_rays_train
 *                     (noises == NULL) + nsr_field_forward + nsr_render_train_forward up to the summation order of that
 *                     kernel's wave scans -- except that nothing is ever dropped: the buffered path zeroes a ray whose samples
 *                     do not fit (offset + count >= M), this one has no M.
 * weights_sum [N], depth [N], image [N, 3 + num_classes]: the raw composite, always written.
 * rgb_map [N,3], depth_norm [N], classes [N, num_classes]: optional, renderer.py:229-233 -- image[:, :3] + (1 - weights_sum),
 * max(depth - near, 0) / (far - near), image[:, 3:].  All NULL, or rgb_map and depth_norm given and classes given exactly when
 * num_classes != 0; anything else -> NSR_ERR_INVALID_ARG.  A ray that misses the box has near == far == FLT_MAX: rgb_map 1,
 * classes 0, depth_norm 0 / 0, as nsr_render_train_forward gives.
 * n_composited: optional device [N] i32, the samples accumulated for each ray (their sum is what this call adds to stats[0]).
 * stats, order, C, H and the remaining contract as nsr_render_rays_infer.  composite outside the enum -> NSR_ERR_INVALID_ARG;
 * C > 16 or num_classes > 13 -> NSR_ERR_UNSUPPORTED. */
enum nsr_stream_composite { NSR_STREAM_INFER = 0, NSR_STREAM_TRAIN = 1 };
int nsr_render_rays_stream(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *rays_o,
                           const float *rays_d, const uint32_t *order, uint32_t N, const float *nears, const float *fars,
                           const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                           float T_thresh, int composite, float *weights_sum, float *depth, float *image, float *rgb_map,
                           float *depth_norm, float *classes, int32_t *n_composited, uint32_t *stats, nsr_stream_t stream);

/* fp32 master tables -> f16 gather copy (the reference's `embeddings.to(torch.half)` under
 * autocast, grid.py:42-43).  n = number of scalars. */
int nsr_cast_f32_to_f16(const float *src, void *dst, uint64_t n, nsr_stream_t stream);

/* Fused Adam (+ optional EMA shadow) over a flat fp32 arena, one pass, grads zeroed on the way
 * out (replaces torch.optim.Adam + zero_grad + torch_ema, trainers/base.py:216-229,420-426).
 * grad_scale_inv multiplies the gradient first (GradScaler unscale). step >= 1.
 * half_copy (f16, may be NULL) receives the updated parameters rounded to half.
 * elem_mask4: bit (i & 3) set <=> element i is trained; others keep parameter and moments (their
 * gradient is still zeroed).  0xF = everything; on the interleaved tables 0x3 = density table only,
 * 0xC = colour table only (stylisation, trainers/style.py:25). */
int nsr_adam_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *ema,
                  void *half_copy, uint64_t n, float lr, float beta1, float beta2, float eps,
                  float grad_scale_inv, float ema_decay, uint32_t step, uint32_t elem_mask4,
                  nsr_stream_t stream);

/* Device-side GradScaler + optimiser bookkeeping (replaces scaler.step(optim) / scaler.update() / scheduler.step(),
 * trainers/base.py:228,420-425 and trainers/style.py:200-204, which read the inf flag back to the host every step).
 * scaler_state: device buffer of 16 32-bit words, kept by the caller across steps:
 *   [0] f32 loss scale (initialise to 65536, GradScaler's default)   [1] i32 growth tracker   [2] u32 found_inf
 *   [3] u32 optimiser steps taken   [4] u32 steps skipped   [5] u32 EMA updates made   [8..13] this step's values for
 *   nsr_adam_step_scaled (skip flag, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), 1 / scale, lr, EMA decay); other words
 *   reserved, initialise to 0.
 * One optimiser step =
 *   nsr_grad_check        per trained region: sets found_inf if any element selected by elem_mask4 is inf / nan
 *                         (GradScaler.unscale_'s check; untrained regions are not looked at, so data-parallel ranks
 *                         that all-reduce only the trained regions take the same decision);
 *   nsr_scaler_update     one thread: skip decision, scale *= backoff and tracker = 0 on inf, else step count += 1,
 *                         tracker += 1, scale *= growth every growth_interval clean steps; lr = lr_base *
 *                         0.1^((t-1) / lr_decay_steps) (LambdaLR advanced only on steps that were not skipped;
 *                         lr_decay_steps <= 0: constant) and Adam's bias corrections for step t, in double precision;
 *                         enabled == 0: never skips, scale stays 1 (GradScaler(enabled=False)); clears found_inf;
 *                         ema_decay_max >= 0: torch_ema's schedule, num_updates += 1 and decay = min(ema_decay_max,
 *                         (1 + n) / (10 + n)) on every call (skipped steps included); < 0: no EMA;
 *   nsr_adam_step_scaled  per trained region: nsr_adam_step with those device-side scalars; on a skipped step the
 *                         parameters and moments stay, the gradient is still zeroed and the EMA still moves
 *                         (ema.update() is unconditional, base.py:426).  half_copy covers the first half_n elements.
 * Nothing is read on the host: legal under stream capture. */
int nsr_grad_check(const float *grads, uint64_t n, uint32_t elem_mask4, void *scaler_state, nsr_stream_t stream);
int nsr_scaler_update(void *scaler_state, float lr_base, float lr_decay_steps, float beta1, float beta2,
                      float growth_factor, float backoff_factor, uint32_t growth_interval, int enabled,
                      float ema_decay_max, nsr_stream_t stream);
int nsr_adam_step_scaled(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *ema,
                         void *half_copy, uint64_t n, uint64_t half_n, float beta1, float beta2, float eps,
                         uint32_t elem_mask4, const void *scaler_state, nsr_stream_t stream);

/* Lane-packed tables: ONE of the two interleaved hash tables trained alone (the stylisation stage, trainers/style.py:25),
 * its optimiser step sharded across data-parallel ranks.  lane_mask: 0x3 = density table (lanes 0, 1 of every 16-byte row),
 * 0xC = colour table (lanes 2, 3); the trained float2 of row r is packed[2r .. 2r+1].  Stream-ordered, capture-safe
 * (no host read, no allocation).
 *   nsr_lanes_pack         packed[2r..2r+1] = trained lanes of grad row r, r < rows; all four lanes of every row are then
 *                          zeroed (untrained gradients are still zeroed).  grad_arena 16-byte, packed 8-byte aligned.
 *   nsr_lanes_adam(_scaled) Adam + EMA for rows [row_lo, row_hi): grad, exp_avg, exp_avg_sq and packed_out are packed and
 *                          shard-local (element 2 (r - row_lo) + l); ema (may be NULL) holds all four lanes of those rows
 *                          (float4 per row, shard-local), moved as nsr_adam_step moves every element of a trained row.
 *                          arena and half_copy (f16, may be NULL) are the whole tables, updated in place at row r.
 *                          packed_out (may alias grad) receives the rows' trained lanes after the step, skipped or not.
 *                          Arithmetic identical to nsr_adam_step / nsr_adam_step_scaled (host scalars / scaler_state).
 *   nsr_lanes_unpack       rows [row_lo, row_hi) of a gathered packed buffer (indexed by global row) -> their arena lanes
 *                          and all four lanes of half_copy (may be NULL). */
int nsr_lanes_pack(float *grad_arena, uint64_t rows, uint32_t lane_mask, float *packed, nsr_stream_t stream);
int nsr_lanes_adam(float *arena, void *half_copy, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema,
                   float *packed_out, uint64_t row_lo, uint64_t row_hi, uint32_t lane_mask, float lr, float beta1,
                   float beta2, float eps, float grad_scale_inv, float ema_decay, uint32_t step, nsr_stream_t stream);
int nsr_lanes_adam_scaled(float *arena, void *half_copy, const float *grad, float *exp_avg, float *exp_avg_sq,
                          float *ema, float *packed_out, uint64_t row_lo, uint64_t row_hi, uint32_t lane_mask,
                          float beta1, float beta2, float eps, const void *scaler_state, nsr_stream_t stream);
int nsr_lanes_unpack(const float *packed, uint64_t row_lo, uint64_t row_hi, uint32_t lane_mask, float *arena,
                     void *half_copy, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Occupancy-grid update on the device: replaces Renderer.update_state / _compute_occ_sigmas
 * (renderer.py:120-194), which is torch glue with two host reads (`mean_density.item()`, the size of
 * `nonzero(density_grid > 0)`).  One update = nsr_occ_sample_points -> nsr_field_forward (sigma only,
 * rgbs = NULL, on the returned positions) -> nsr_occ_update.  Nothing is read on the host; every call is
 * capture-safe.  Cells are flat indices cas * H^3 + morton(x, y, z): the layout of density_grid [C, H^3]
 * (renderer.py:62-63).  H must be a power of two in 8..512 (a Morton index is below H^3 only then), C <= 8 and
 * C * H^3 < 2^31; any other shape is refused (0 bytes / 0 points / NSR_ERR_INVALID_ARG).
 * ------------------------------------------------------------------------------------------ */
/* device scratch for both calls (the same buffer must be passed to both calls of one update) */
uint64_t nsr_occ_workspace_bytes(uint32_t C, uint32_t H);
/* points of one update: full_update (renderer.py:143-160) C*H^3, one per cell in flat-index order;
 * else (renderer.py:163-181) per cascade H^3/4 uniform cells followed by H^3/4 draws from the occupied ones */
uint32_t nsr_occ_num_points(uint32_t C, uint32_t H, int full_update);
/* xyzs [P,3] f32 = cell centre position 2*c/(H-1)-1 scaled by (b - b/H) plus (u*2-1)*b/H, b = min(2^cas, bound)
 * (renderer.py:130-133); indices [P] i32 = flat cell index (-1: no point -- the occupied half of a cascade whose
 * grid is empty, where the reference's randint(0, 0) raises).  u in [0,1): Philox4x32-10 keyed by `seed`, counter =
 * (point, sequence [+ sequence_dev[0]]) -- the same numbers on every rank; `noise` [P,3] (optional, device)
 * overrides u (tests pin the jitter with it). */
int nsr_occ_sample_points(const float *density_grid, uint32_t C, uint32_t H, float bound, int full_update,
                          uint64_t seed, uint32_t sequence, const uint32_t *sequence_dev, const float *noise,
                          float *xyzs, int32_t *indices, void *workspace, nsr_stream_t stream);
/* sigmas [P] f32 = field densities (already x density_scale) at those points.  Applies renderer.py:183-189:
 * tmp_grid = -1 except tmp_grid[indices] = sigmas; where grid >= 0 and tmp >= 0: grid = max(grid * decay, tmp);
 * mean_density[0] (device f32) = mean(clamp(grid, 0)); bitfield = packbits(grid, min(mean, density_thresh)).
 * sequence_dev (optional) is incremented, so a captured graph draws fresh jitter on every replay. */
int nsr_occ_update(float *density_grid, const float *sigmas, const int32_t *indices, uint32_t P, uint32_t C,
                   uint32_t H, int full_update, float density_decay, float density_thresh, uint8_t *bitfield,
                   float *mean_density, uint32_t *sequence_dev, void *workspace, nsr_stream_t stream);

/* Untrained cells: marks every cell that fewer than min_views of the F training cameras see with density_grid = -1, the
 * state nsr_occ_update never leaves (its valid mask is grid >= 0) and the occupied-cell list never names, and clears the
 * cell's bit in `bitfield` (optional; the other bits of the byte are kept).  torch-ngp's mark_untrained_grid /
 * instant-ngp's mark_untrained_density_grid; the reference has the state but no producer.
 *
 * poses [F,3,4] f32 row-major (device), [R | t] with R taken as ORTHONORMAL (camera to world, as nsr_generate_rays_frames
 * reads them); camera_flip as there.  The frustum is x_lo <= x' / z' <= x_hi, y_lo <= y' / z' <= y_hi in the pinhole
 * coordinates of the frame's outer pixel edges ((0 - cx) / fx .. (w - cx) / fx, likewise y); no near or far limit.
 *
 * Geometry, all fp64, no contraction, every operation an IEEE + - x (sqrt on the host) in this order:
 *   cell cas * H^3 + morton(ix, iy, iz):  b = min(2^cas, (double)bound), half = b / H,
 *     centre X_a = b (2 i_a + 1 - H) / H  (the centre of the march's cell and of the update's),
 *     rho = (margin_cells * half) * sqrt(3.0);
 *   frame [R | t] (f32 widened):  d = X - t,  q_k = (R[0][k] d_0 + R[1][k] d_1) + R[2][k] d_2  (q = R^T (X - t)),
 *     x' = q_0 f0, y' = q_1 f1, z' = q_2 f2 with f0, f1, f2 = +-1 from camera_flip bits 2, 1, 0: the inverse of the ray
 *     direction R (x f0, y f1, f2) of nsr_generate_rays;
 *   the frame SEES the cell iff   z' + rho > 0
 *                            and  x' - x_hi z' <= rho sqrt(1 + x_hi^2)   and  x_lo z' - x' <= rho sqrt(1 + x_lo^2)
 *                            and  y' - y_hi z' <= rho sqrt(1 + y_hi^2)   and  y_lo z' - y' <= rho sqrt(1 + y_lo^2),
 *   i.e. the sphere of radius rho around the centre reaches into every half-space of the frustum.
 * Conservative: with margin_cells = 1, rho is the cell's half-diagonal, so every point of the cell lies within rho of the
 * centre; R is orthonormal, so q = R^T (X - t) keeps distances; a point of the cell inside the frustum lies inside every
 * half-space, and the centre is then at most rho outside each (the right-hand sides divide by the normals' lengths).  So a
 * cell with any point inside a frustum is seen; cells near a frustum's edges or corners may be seen without touching it.
 *
 * count = the number of frames that see the cell (all F are counted); counts [C*H^3] i32 (optional) receives it.
 *   count <  min_views: grid = -1.0f, bit cleared;
 *   count >= min_views: a grid value < 0 becomes 0.0f (a cell the cameras now see is trainable again), every other value
 *     keeps its bits (NaN and -0.0f included) and the bit is kept.
 * A second call with the same arguments changes nothing.  n_untrained [C] u32 (optional) is WRITTEN with the number of
 * cells per cascade this call left at -1 (zeroed by a kernel of the call, then integer atomics of block sums: the same
 * value on every run).  Reads nothing on the host, uses no workspace, capture-safe.  Shapes as for every nsr_occ_* call;
 * also refused (NSR_ERR_INVALID_ARG): F == 0, min_views == 0, margin_cells < 0 or NaN, x_lo >= x_hi, y_lo >= y_hi or a
 * frustum bound that is not finite, density_grid or counts not 16-byte aligned. */
int nsr_occ_mark_untrained(float *density_grid, uint8_t *bitfield, uint32_t C, uint32_t H, float bound, const float *poses,
                           uint32_t F, double x_lo, double x_hi, double y_lo, double y_hi, int camera_flip,
                           double margin_cells, uint32_t min_views, int32_t *counts, uint32_t *n_untrained,
                           nsr_stream_t stream);

/* Ray generation on the device (nerf_lib.py:69-142 + common.py:139-147): pixel centres
 * (x + 0.5), camera-frame direction ((i-cx)/fx, (j-cy)/fy, 1) * flip, R * d, normalise.
 * pose [4,4] f32 row-major (device).  pix [N] i32 1-D pixel ids (row-major, y * w + x) or NULL
 * for all w*h pixels in order (then N == w*h).  flip bits as camera_flip (nerf_lib.py:121). */
int nsr_generate_rays(const float *pose, uint32_t w, uint32_t h, float fx, float fy, float cx,
                      float cy, int camera_flip, const int32_t *pix, uint32_t N, float *rays_o,
                      float *rays_d, nsr_stream_t stream);

/* Backward of nsr_generate_rays with respect to the pose (same leading arguments): grad_pose [3,4] f32 row-major is WRITTEN,
 * grad_pose[:, 3] = sum_n grad_rays_o[n] and, with c_n the pixel's camera-frame direction after the flip, v_n = R c_n and
 * d_n = v_n / |v_n|:  grad_pose[:, :3] = sum_n ((I - d_n d_n^T) grad_rays_d[n] / |v_n|) c_n^T.
 * Terms and sums are formed in fp64 and rounded once; block tree + a fixed-order final pass (no atomics, no counter, nothing
 * of the workspace is read that this call did not write): two calls give the same bits.  Capture-safe.
 * workspace: nsr_generate_rays_backward_workspace_bytes(N) bytes, 8-byte aligned. */
uint64_t nsr_generate_rays_backward_workspace_bytes(uint32_t N);
int nsr_generate_rays_backward(const float *pose, uint32_t w, uint32_t h, float fx, float fy, float cx, float cy,
                               int camera_flip, const int32_t *pix, uint32_t N, const float *grad_rays_o,
                               const float *grad_rays_d, void *workspace, float *grad_pose, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mixed-frame ray batches: the rays of many cameras in one training step.  A batch is S segments of K rays each
 * (N = S * K), ray n belongs to segment n / K, segment s names one frame seg_frame[s] in [0, F); frames may repeat
 * (K = 1: a frame per ray).  S, K and F are host integers; seg_frame [S] i32 and pix [N] i32 live on the device and may
 * change between replays of a captured graph.  Every call is capture-safe.
 * ------------------------------------------------------------------------------------------ */
/* nsr_generate_rays with a pose per segment: poses [F,3,4] f32 row-major (device).  Row n is bit-identical to
 * nsr_generate_rays called with the pose of frame seg_frame[n / K] and pix[n] (the same operations in the same order, no
 * contraction).  A segment whose seg_frame entry is outside [0, F) gets NaN origins and directions -- the march and the field
 * treat NaN positions as out of range -- and no pose is read for it. */
int nsr_generate_rays_frames(const float *poses, uint32_t F, uint32_t w, uint32_t h, float fx, float fy, float cx, float cy,
                             int camera_flip, const int32_t *seg_frame, const int32_t *pix, uint32_t S, uint32_t K,
                             float *rays_o, float *rays_d, nsr_stream_t stream);

/* Its backward with respect to the poses (same leading arguments): grad_poses [F,3,4] f32 row-major is WRITTEN for every
 * frame, exact zeros for a frame that no segment names; a segment whose entry is outside [0, F) contributes nothing.  Per
 * frame the sums of nsr_generate_rays_backward over the rays of the segments naming it.  Per-ray terms in fp64 as there;
 * reduction order: per segment block trees (below 64 rays per segment: one thread per segment, rays in order), the segment's
 * block partials in ascending order, then per frame the segments naming it in ascending s; all in fp64, rounded to fp32 once.
 * No atomics, no counters, nothing of the workspace is read that this call did not write: two calls give the same bits.
 * workspace: nsr_generate_rays_frames_backward_workspace_bytes(F, S, K) bytes, 8-byte aligned. */
uint64_t nsr_generate_rays_frames_backward_workspace_bytes(uint32_t F, uint32_t S, uint32_t K);
int nsr_generate_rays_frames_backward(const float *poses, uint32_t F, uint32_t w, uint32_t h, float fx, float fy, float cx,
                                      float cy, int camera_flip, const int32_t *seg_frame, const int32_t *pix, uint32_t S,
                                      uint32_t K, const float *grad_rays_o, const float *grad_rays_d, void *workspace,
                                      float *grad_poses, nsr_stream_t stream);

/* Lens refinement: the rays of a mixed-frame batch through a lens that lives in device memory and may change between the
 * replays of a captured graph.  lens [6] f32 = (fx, fy, cx, cy, k1, k2).  Per ray, with (i, j) the pixel centre and f0..f2 the
 * camera flip's signs as in nsr_generate_rays, in fp32 without contraction, in this order:
 *   x  = (i - cx) / fx;  y = (j - cy) / fy
 *   r2 = x*x + y*y
 *   s  = 1.0f + r2 * (k1 + r2 * k2)
 *   c  = ((x*s)*f0, (y*s)*f1, f2)             then R c and the normalisation of nsr_generate_rays
 * The polynomial radial model applied in the UNPROJECTION direction (pixel to ray): closed form, no iterative undistortion.
 * k1, k2 are therefore NOT OpenCV's forward (ray to pixel) coefficients.  With k1 = k2 = 0, s is exactly 1 and every row is
 * bit-identical to nsr_generate_rays_frames with the same fx, fy, cx, cy.  Segments as there: an entry of seg_frame outside
 * [0, F) gives NaN rows and reads no pose.  A single pose is F = S = 1, K = N with seg_frame = {0}. */
int nsr_generate_rays_lens(const float *poses, uint32_t F, uint32_t w, uint32_t h, const float *lens, int camera_flip,
                           const int32_t *seg_frame, const int32_t *pix, uint32_t S, uint32_t K, float *rays_o, float *rays_d,
                           nsr_stream_t stream);

/* Its backward (same leading arguments).  grad_lens [6] f32 is WRITTEN; grad_poses [F,3,4] f32 is written for every frame
 * unless it is NULL (only the lens gradient is wanted).  Per ray in fp64, from the f32 inputs: x, y, r2, s and c as above,
 * v = R c, d = v / |v|, h = (I - d d^T) g_d / |v|; the twelve pose terms are h c^T and g_o as in nsr_generate_rays_backward.
 * With q = R^T h, gX = q0 f0, gY = q1 f1, m = gX x + gY y, s' = k1 + 2 k2 r2, gx = gX s + 2 m s' x, gy = gY s + 2 m s' y:
 *   d fx = -gx x / fx   d fy = -gy y / fy   d cx = -gx / fx   d cy = -gy / fy   d k1 = m r2   d k2 = m r2^2
 * Reduction: the segment-to-block mapping and the order of nsr_generate_rays_frames_backward with eighteen sums per block; the
 * pose rows per frame over the segments naming it in ascending s, the lens row over every segment naming a frame in [0, F) in
 * ascending s; fp64 throughout, rounded to fp32 once.  A segment outside [0, F) adds nothing to either result; a frame no
 * segment names gets exact zeros.  With k1 = k2 = 0 the pose rows are nsr_generate_rays_frames_backward's bit for bit.  No
 * atomics, no counters, nothing of the workspace is read that this call did not write: two calls and the replays of a
 * captured graph give the same bits.
 * workspace: nsr_generate_rays_lens_backward_workspace_bytes(F, S, K) bytes, 8-byte aligned. */
uint64_t nsr_generate_rays_lens_backward_workspace_bytes(uint32_t F, uint32_t S, uint32_t K);
int nsr_generate_rays_lens_backward(const float *poses, uint32_t F, uint32_t w, uint32_t h, const float *lens, int camera_flip,
                                    const int32_t *seg_frame, const int32_t *pix, uint32_t S, uint32_t K,
                                    const float *grad_rays_o, const float *grad_rays_d, void *workspace, float *grad_poses,
                                    float *grad_lens, nsr_stream_t stream);

/* Draws a batch on the device: UNIFORM WITH REPLACEMENT (the reference draws without replacement inside one frame; duplicates
 * in a 4 096-of-762 048 draw do not matter to a mean loss).  P = w * h pixels per frame.  Philox4x32-10 keyed by `seed`, with
 * seq = sequence + (sequence_dev ? sequence_dev[0] : 0):
 *   segment s:          r = philox(s, seq, 2, stream_id),  seg_frame[s] = umulhi(r.x, F); with fixed_frames ([S] i32, device,
 *                       optional) seg_frame[s] = fixed_frames[s] and no draw is made
 *   ray n = s * K + k:  q = philox(n, seq, 3, stream_id),  pix[n] = umulhi(q.x, P),  rows[n] (int64) = seg_frame[s] * P + pix[n],
 *                       the ray's row of a [F * P, ...] target table (a fixed frame outside [0, F) counts as frame 0 in rows
 *                       only, so that no consumer of rows reads out of bounds)
 * stream_id: the data-parallel rank -- ranks draw distinct batches from one seed.  advance != 0 (needs sequence_dev): after the
 * draw, on the same stream, a kernel of its own increments sequence_dev[0], so a captured graph draws a fresh batch on every
 * replay, like nsr_occ_update. */
int nsr_draw_frame_batch(uint32_t F, uint32_t P, uint32_t S, uint32_t K, uint64_t seed, uint32_t sequence,
                         uint32_t *sequence_dev, uint32_t stream_id, const int32_t *fixed_frames, int advance,
                         int32_t *seg_frame, int32_t *pix, int64_t *rows, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Error-map importance sampling (instant-ngp's error map): pixels drawn in proportion to a coarse per-frame map of the running
 * training error, every ray weighted by (uniform pdf) / (pdf of its draw), so that mean(weight * loss) still estimates the
 * uniform mean loss.  Everything that decides a draw is INTEGER arithmetic (atomic integer sums are exact in any order): two
 * runs, two ranks and a restatement on the host reach the same bits.  All calls are capture-safe and read nothing on the host.
 *
 * Grid: a w x h frame is cut into cell x cell pixel cells, gw = ceil(w / cell), gh = ceil(h / cell), G = gw * gh; cell g has
 * column gx = g % gw and row gy = g / gw, real extent cw = min(cell, w - gx * cell) by ch = min(cell, h - gy * cell) and
 * npix = cw * ch pixels; pixel p (row-major, y * w + x) lies in cell (y / cell) * gw + x / cell.  P = w * h.
 * State, all on the device, caller-allocated: err [F,G] f32 (running squared error per cell), acc_sum [F,G] u64 and
 * acc_cnt [F,G] u32 (this step's accumulators, zero between steps), prefix [F,G] u64, frame_prefix [F] u64 (8-byte aligned).
 * cell == 0, F, w or h == 0, P or F * G past 31 bits -> NSR_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------------------------ */
/* Adds the rays' errors to the accumulators.  Ray n (segment n / K, frame f = seg_frame[n / K], pixel p = pix[n]) is skipped when
 * f is outside [0, F), p outside [0, P), or ray_err[n] is NaN or negative.  Otherwise, in fp32,
 *   a = (u64) min(floor(ray_err[n] * 2^20), 2^22)
 * is added to acc_sum[f, cell of p] and 1 to acc_cnt[f, cell of p] with integer atomics (a wave adds up the rays that share a
 * cell first, for up to four distinct cells: a frame walked in 8 x 8 tiles makes one request per wave, not 64). */
int nsr_error_map_accumulate(uint32_t F, uint32_t w, uint32_t h, uint32_t cell, const int32_t *seg_frame, const int32_t *pix,
                             const float *ray_err, uint32_t S, uint32_t K, uint64_t *acc_sum, uint32_t *acc_cnt, nsr_stream_t stream);

/* Folds the accumulators into err and rebuilds the prefixes (two launches: a workgroup per frame, then one workgroup over the
 * frames' totals).  Per cell with acc_cnt > 0, no contraction, in this order:
 *   mean = (f32)((f64)acc_sum / (f64)acc_cnt * 2^-20);   err = err + decay * (mean - err);   acc_sum = acc_cnt = 0
 * (other cells keep err bit for bit).  Then for every cell  q = (u32) min(floor(err * quant_scale), 2^18)  in fp32, 0 when the
 * product is NaN or negative; the cell's mass is npix * q (u64); prefix[f, g] = sum of the masses of cells 0..g of frame f
 * (inclusive), the frame's total is prefix[f, G - 1], and frame_prefix[f] = sum of the totals of frames 0..f (inclusive).
 * decay outside [0, 1] or quant_scale <= 0 -> NSR_ERR_INVALID_ARG. */
int nsr_error_map_rebuild(uint32_t F, uint32_t w, uint32_t h, uint32_t cell, float decay, float quant_scale, float *err,
                          uint64_t *acc_sum, uint32_t *acc_cnt, uint64_t *prefix, uint64_t *frame_prefix, nsr_stream_t stream);

/* nsr_draw_frame_batch (same Philox calls, seed, seq, stream_id, fixed_frames, advance, seg_frame, pix, rows) with the pixels,
 * and optionally the frames, drawn from the map; weights [N] f32.  u = uniform_mix in [0, 1] (else NSR_ERR_INVALID_ARG),
 * t = round(u * 2^32) as a 64-bit integer, mulhi64(x, m) = (x * m) >> 64, total_f = prefix[f, G - 1],
 * grand = frame_prefix[F - 1]; "first above" is the first index whose inclusive prefix exceeds the target.
 *   segment s:  r = philox(s, seq, 2, stream_id), uniform frame fu = umulhi(r.x, F).
 *       fixed_frames: seg_frame[s] = fixed_frames[s], frame factor 1.
 *       frames_by_error == 0, or grand == 0: seg_frame[s] = fu, frame factor 1.
 *       else: seg_frame[s] = fu if r.y < t, otherwise first above mulhi64(r.z * 2^32 + r.w, grand) in frame_prefix;
 *             frame factor = 1 / (u + (1 - u) * ((f32)F * (f32)total_f) / (f32)grand).
 *   ray n of frame f:  r = philox(n, seq, 3, stream_id), uniform pixel pu = umulhi(r.x, P).
 *       f outside [0, F) (a fixed frame), or total_f == 0: pix[n] = pu, pixel factor 1.
 *       else: pix[n] = pu if r.y < t; otherwise q = philox(n, seq, 4, stream_id), cell g = first above
 *             mulhi64(q.x * 2^32 + q.y, total_f) in prefix[f, :], and pix[n] = (gy * cell + umulhi(q.w, ch)) * w + gx * cell +
 *             umulhi(q.z, cw).  With g the cell of pix[n] (either branch) and q_g = (prefix[f, g] - prefix[f, g - 1]) / npix_g:
 *             pixel factor = 1 / (u + (1 - u) * ((f32)q_g * (f32)P) / (f32)total_f).
 *   weights[n] = pixel factor * frame factor; each factor in fp32, no contraction, evaluated as written: the product in the
 *   inner parentheses, times (1 - u), divided, plus u, reciprocal.  rows[n] as in nsr_draw_frame_batch.
 * u == 1 gives nsr_draw_frame_batch's seg_frame, pix and rows bit for bit and weights of exactly 1. */
int nsr_draw_frame_batch_error(uint32_t F, uint32_t w, uint32_t h, uint32_t cell, const uint64_t *prefix,
                               const uint64_t *frame_prefix, float uniform_mix, int frames_by_error, uint32_t S, uint32_t K,
                               uint64_t seed, uint32_t sequence, uint32_t *sequence_dev, uint32_t stream_id,
                               const int32_t *fixed_frames, int advance, int32_t *seg_frame, int32_t *pix, int64_t *rows,
                               float *weights, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Total variation of the hash-grid tables (torch-ngp's GridEncoder.grad_total_variation): the gradient of a squared-difference
 * smoothness term between neighbouring lattice vertices, added into the table gradient after the backward and before the
 * optimiser step; optionally the term's value.  Additive: the ABI version stays.
 *
 * Table: `rows` rows of row_floats fp32 lanes (1, 2, 4 or 8): 4 for the fused model's arena ([row][enc][feat]), C for a
 * stand-alone GridEncoder.  Levels are (offsets, L, S, H, gridtype) as everywhere else (nsr_grid_resolutions gives res_l); the
 * vertices of level l are (x, y, z) with 0 <= x, y, z <= res_l, V_l = (res_l + 1)^3 of them (64-bit on the host), and the row
 * of a vertex is offsets[l] + the row the forward gathers it from (dense or hashed, style 0).
 *
 * Loss, with lambda [row_floats] HOST floats, one weight per lane k:
 *   TV_{l,k} = (1 / V_l) * sum over the edges (a, a + e_d) inside the lattice of (t[row(a)][k] - t[row(a + e_d)][k])^2
 *   loss     = sum_l sum_k lambda_k * TV_{l,k}
 * Estimator: level l makes n_l = min(n_samples, V_l) draws of a vertex a.
 *   sweep   (n_samples >= V_l): draw i is x = i % (res+1), y = (i / (res+1)) % (res+1), z = i / (res+1)^2: every vertex once,
 *           the gradient is exact
 *   sampled (otherwise): r = philox(i, seq, 5, (stream_id << 8) | l) keyed by `seed` (the Philox4x32-10 of nsr_draw_frame_batch,
 *           whose calls use counter words 0..4), x = umulhi(r.x, res+1), y = umulhi(r.y, res+1), z = umulhi(r.z, res+1)
 *   seq = sequence + (sequence_dev ? sequence_dev[0] : 0); advance != 0 (needs sequence_dev): after the draws, on the same
 *   stream, a kernel of its own increments sequence_dev[0], so a captured graph draws afresh on every replay.  stream_id: the
 *   data-parallel rank.
 * Gradient: each draw a adds, to grad[row(a)][k] only (the fp32 atomic of nsr_grid_encode_backward),
 *   c_{l,k} * scale * sum over d and s = +-1 with 0 <= a_d + s <= res_l of (t[row(a)][k] - t[row(a + s e_d)][k])
 *   c_{l,k} = (float)(2.0 * lambda_k / n_l), formed in fp64 on the host and rounded once;
 *   scale = scale_host * (scale_dev ? scale_dev[0] : 1), scale_dev the device loss scale.
 *   Unbiased; summed over all vertices it is exactly d loss / d t[row], collisions included (each edge is seen once from
 *   either end).  In fp32: the differences, summed as ((x- + x+) + (y- + y+)) + (z- + z+), times the rounded c * scale.
 *   Lanes with lambda_k == 0 are not written (their bits stay); levels whose bit of level_mask is clear are skipped.
 * value (optional, device double [L][row_floats], 8-byte aligned):
 *   value[l][k] = (1 / n_l) * sum over the draws and the d with a_d + 1 <= res_l of (t[row(a)][k] - t[row(a + e_d)][k])^2,
 *   differences and squares in fp64 from the fp32 entries, summed without atomics in an order fixed by (L, n_samples, the
 *   levels): per-workgroup partials in `workspace` (nsr_grid_tv_workspace_bytes(L, n_samples, row_floats) bytes, 8-byte
 *   aligned, needed iff value), then one ordered pass.  Two calls give the same bits.  Lanes with lambda_k == 0 and masked
 *   levels report 0.  grad_tables == NULL with value given computes the value only.
 * tables must be aligned to a row (16 bytes from row_floats = 4 on).  NULL tables, lambda or offsets, neither grad_tables nor
 * value, value without workspace, row_floats outside {1, 2, 4, 8}, L == 0 or L > 32, n_samples == 0, gridtype > 1, or advance
 * without sequence_dev -> NSR_ERR_INVALID_ARG before anything touches a device.  Capture-safe, no host read.
 * ------------------------------------------------------------------------------------------ */
uint64_t nsr_grid_tv_workspace_bytes(uint32_t L, uint32_t n_samples, uint32_t row_floats);
int nsr_grid_tv(const float *tables, float *grad_tables, uint32_t row_floats, const float *lambda, const int32_t *offsets,
                uint32_t L, float S, uint32_t H, uint32_t gridtype, uint32_t level_mask, uint32_t n_samples, uint64_t seed,
                uint32_t sequence, uint32_t *sequence_dev, uint32_t stream_id, int advance, float scale_host,
                const float *scale_dev, double *value, void *workspace, nsr_stream_t stream);

/* Structural similarity (Wang et al. 2004 in the form 3DGS and pytorch-ssim use) of two H x W RGB images, and its gradient
 * towards the first: value, optional map, optional gradient in one call.
 * Layout: both images are pixel-major rows read where they are: channel c of pixel (y, x) is
 *   img[(y * img_pitch + x) * img_stride + c]            stride in {3, 4} floats a pixel (the fourth is never read),
 *   target[(y * target_pitch + x) * target_stride + c]   pitch >= W pixels an image row (a patch of a larger frame in place)
 * 4-byte aligned, 16-byte aligned for stride 4.
 * Definition, per channel, data range 1, C1 = 0.01^2, C2 = 0.03^2, x = img, y = target:
 *   window  g[i] = exp(-(i-5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1 in fp64, then rounded to f32; G* is the
 *           separable 11x11 convolution with these weights, zero padding of 5; rows first, then columns, each sum an f32 fmaf
 *           chain over the taps in ascending order
 *   mu_x = G*x, mu_y = G*y, sxx = G*(x x) - mu_x^2, syy = G*(y y) - mu_y^2, sxy = G*(x y) - mu_x mu_y     (no clamping)
 *   m = ((2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1)) * ((2 sxy + C2) / (sxx + syy + C2))                  (f32)
 *   The window sums are taken of x' = x - 1/2 and y' = y - 1/2 inside the image (zero outside, as the padding of x is) and the
 *   same quantities formed from them, with g1 = G*1 the window mass inside the image (fp64) and d = 1 - g1:
 *   mu_x = G*x' + g1/2, sxx = [G*(x'x') - (G*x')^2] + (G*x') d + g1 d/4, sxy = [G*(x'y') - G*x' G*y'] + (G*x' + G*y') d/2 + g1 d/4:
 *   the cancellation in the variances, which sets the f32 error of m, is then between numbers of size 1/4 at most.
 *   valid == 0 ('same'):  every pixel is counted, count = 3 H W
 *   valid == 1 ('valid'): pixels whose whole window lies inside the image, 5 <= x < W - 5 and 5 <= y < H - 5,
 *                         count = 3 (H - 10)(W - 10); needs H, W >= 11
 * out [4] (device fp64, 8-byte aligned): the mean of m over the counted pixels of all channels, then the three channel means.
 * ssim_map (optional) [H*W, 3] f32, rows in image order: m, 0 where the pixel is not counted.
 * grad (optional) [H*W, 3] f32: with A = dm/dmu_x - 2 mu_x dm/dsxx - mu_y dm/dsxy, B = dm/dsxx, C = dm/dsxy at the counted
 *   pixels and 0 elsewhere,
 *   unit(q) = ((G*A)(q) + 2 x(q) (G*B)(q) + y(q) (G*C)(q)) * (float)(1 / count)        = dSSIM / dx(q), in f32, uncontracted
 *   grad(q) = (coef * (scale ? scale[0] : 1)) * unit(q)                                two f32 products
 *   scale: 0-dim f32 DEVICE pointer or NULL (LossScaler.scale_tensor, as in nsr_recon_loss); a D-SSIM loss
 *   lambda * (1 - SSIM) passes coef = -lambda * factor.  No gradient towards target.  For identical images m == 1 and
 *   grad == 0 exactly.
 * Order of the sums of m (fp64; no atomics; two calls and the replays of a captured graph give the same bits in value, map
 * and gradient): one workgroup of 256 threads per 32x32 tile and channel; thread t owns column t % 32 and rows
 * 4 (t / 32) .. + 3 of the tile and adds its pixels in ascending row; butterfly over the 64 lanes (lane ^ 32, 16, 8, 4, 2, 1);
 * the four waves in ascending order -> partial[c][tile], tiles in row-major order.  Final pass, one block of 256 threads:
 * thread t adds partial[c][t], partial[c][t + 256], ... in that order, then wave and block as above; out[1 + c] =
 * s_c / (count / 3), out[0] = ((s_0 + s_1) + s_2) / (count / 3) / 3.
 * workspace: nsr_ssim_workspace_bytes(H, W, want_grad) bytes, 8-byte aligned (want_grad != 0 iff grad is given: the
 * partials, then A, B, C as nine f32 planes); nothing of it is read that this call did not write.  The size is 0 for a
 * shape that nsr_ssim refuses.
 * Refused with NSR_ERR_INVALID_ARG, before any pointer is looked at: H == 0, W == 0, H * W > 2^30 or H > 32 * 65535,
 * valid > 1, a stride outside {3, 4}, a pitch < W, valid with H < 11 or W < 11; then a NULL img, target, out or workspace,
 * a misaligned pointer, grad or ssim_map overlapping an input or each other.  Nothing is written then.
 * No host read, no allocation, capture-safe. */
uint64_t nsr_ssim_workspace_bytes(uint32_t H, uint32_t W, uint32_t want_grad);
int nsr_ssim(const float *img, uint32_t img_stride, uint32_t img_pitch, const float *target, uint32_t target_stride,
             uint32_t target_pitch, uint32_t H, uint32_t W, uint32_t valid, float coef, const float *scale, double *out,
             float *ssim_map, float *grad, void *workspace, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mesh export: the iso-surface of a scalar volume by naive surface nets (Gibson 1998), as an indexed triangle mesh
 * (csrc/surface_nets.hip; torch-ngp's save_mesh does this with marching cubes on the host).  Additive: the ABI version stays.
 * The output is a pure function of the input: no atomics, two calls give the same bits.
 *
 * Volume vol[i,j,k] f32, C-contiguous [R0,R1,R2] (k fastest), 2 <= R_a <= 1024.  Lattice point p(i,j,k) = lo + (i step_x,
 * j step_y, k step_z), each coordinate lo_a + (float)i * step_a in f32 without contraction; lo [3], step [3] are HOST floats,
 * step = (hi - lo) / (R - 1) formed by the caller in f32.
 * A point is INSIDE iff vol > iso (strict): a NaN and a value equal to iso are outside.
 * Cell (cx,cy,cz), 0 <= c_a <= R_a - 2, linear index (cx (R1-1) + cy)(R2-1) + cz; its corner q = 4 dx + 2 dy + dz is the point
 * (cx+dx, cy+dy, cz+dz).  A cell is ACTIVE iff its 8 corners are neither all inside nor all outside.
 *
 * Vertices.  Every active cell has one vertex; its id is the rank of the cell among the active cells in linear cell order.
 *   The 12 edges as (corner, corner), in this order:
 *     along x (0,4) (1,5) (2,6) (3,7), along y (0,2) (1,3) (4,6) (5,7), along z (0,1) (2,3) (4,5) (6,7).
 *   An edge whose ends differ in inside-ness crosses: with a its outside end, b its inside end and va, vb their values,
 *     t = (iso - va) / (vb - va); if not 0 <= t <= 1 (va a NaN, or -inf against +inf): t = 1/2
 *     crossing point: the coordinate along the edge's axis is pa + t * (pb - pa), the two others are the corners' own.
 *   vertex = (sum of the crossing points, added to +0 in edge order, coordinate by coordinate) / (float)(their number).
 *   All in f32, every operation rounded once (no contraction, IEEE division).
 * Faces.  Cell (cx,cy,cz) owns the three lattice edges that leave its corner 0 along +x, +y, +z.  The owned edge along axis a
 *   emits one quad iff its ends differ in inside-ness and the cell's two other coordinates are both >= 1 (the four cells around
 *   the edge then exist, and all are active).  With (u, w) the axes after a in the cyclic order x, y, z, the quad's corners are
 *   the vertices of the cells
 *     v0 = c - e_u - e_w, v1 = c - e_w, v2 = c, v3 = c - e_u        (counter-clockwise seen from the axis' positive end)
 *   in this order when corner 0 is the inside end and as (v0, v3, v2, v1) otherwise, so that the right-hand normal points from
 *   the inside end to the outside end (along -grad of the volume, the convention of nsr_field_density_gradient's unit normal).
 *   A quad is the triangles (q0,q1,q2), (q0,q2,q3).  Faces are ordered by (owning cell's linear index, axis).
 *   The mesh is a closed oriented 2-manifold wherever the surface stays off the lattice's boundary; where it reaches it the
 *   mesh is open (edges on the upper boundary planes are owned by no cell, those on the lower ones miss a neighbour).
 *
 * Two calls, because the output sizes are known only after a count:
 *   nsr_surface_nets_count: fills `workspace` (nsr_surface_nets_workspace_bytes(R0,R1,R2) bytes, 16-byte aligned: a header
 *     {V, Q, R0, R1, R2}, the scanned per-block offsets, cell_vertex int32 [cells]) and writes counts_out[0] = V (vertices),
 *     counts_out[1] = Q (quads; 2 Q triangles) on the device.  No host read, capture-safe.
 *   nsr_surface_nets_emit: from the same vol, iso and the workspace the count left: verts [V,3] f32 and faces [2 Q,3] int32.
 *     It READS THE HEADER BACK ON THE HOST (20 bytes, one stream synchronisation -- the one entry point of the library that
 *     does; it is not legal inside a stream capture) and refuses a V, Q or shape that is not the workspace's before anything
 *     is launched: V and Q size the caller's outputs.  V == 0 (then Q == 0) is a no-op success; verts and faces may be NULL
 *     where their size is 0.
 * NSR_ERR_INVALID_ARG before any launch: an R_a outside [2, 1024] (checked first; the workspace size is 0 then), a NULL vol,
 * workspace, counts_out, lo or step, a NULL verts with V > 0 or faces with Q > 0, a pointer not aligned to 4 bytes (workspace:
 * 16), V > cells, Q > 3 cells, Q > 0 with V == 0, or the mismatch above.
 * ------------------------------------------------------------------------------------------ */
uint64_t nsr_surface_nets_workspace_bytes(uint32_t R0, uint32_t R1, uint32_t R2);
int nsr_surface_nets_count(const float *vol, uint32_t R0, uint32_t R1, uint32_t R2, float iso, void *workspace,
                           uint32_t *counts_out, nsr_stream_t stream);
int nsr_surface_nets_emit(const float *vol, uint32_t R0, uint32_t R1, uint32_t R2, float iso, const float *lo, const float *step,
                          void *workspace, uint32_t V, uint32_t Q, float *verts, int32_t *faces, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mesh cleaning: connected components of an indexed triangle mesh, their statistics, and a filter that drops whole components
 * (csrc/mesh_clean.hip; torch-ngp's clean_mesh does this on the host after its marching cubes).  Additive: the ABI version stays.
 * Every output is a pure function of the input: two calls give the same bits.
 *
 * Mesh: verts f32 [V,3], faces int32 [F,3], 0 <= V, F < 2^31.
 * Components.  Two vertices are joined when one face holds both; components are the transitive closure of that relation.
 *   label[v] = the SMALLEST vertex id of v's component; a vertex in no face is a component of its own, label[v] = v.
 *   Degenerate faces (repeated indices) and duplicate faces are ordinary input.
 * Bad faces.  A face with any index outside [0, V) joins nothing, belongs to no component, is never emitted and is counted in
 *   *bad_faces (a device integer).  No kernel dereferences such an index.
 * Statistics, read at the roots (the r with label[r] == r); the arrays are indexed by vertex id and hold 0, 0 and the empty
 *   box (+inf, -inf) at every vertex that is no root:
 *     n_verts[r]; n_faces[r] (a face counts for the component of its vertices); lo[r], hi[r]: the exact f32 minimum and maximum
 *     of the component's vertices, coordinate by coordinate (-0 orders below +0; vertices are assumed finite).
 *   Integer adds, mins and maxes are order-free, so these kernels use atomics and are deterministic all the same.
 * Filter.  keep [V] uint8, read at the roots: the caller's decision per component (the keep rule of nerfstyle_amd/mesh.py:
 *   n_faces >= min_faces; dx^2 + dy^2 + dz^2 >= min_diagonal^2 with d = hi - lo, in f32 in this written order; optionally the
 *   k components of the most faces among those, ties to the smaller label).  Vertices and faces of components that are not kept
 *   go; the survivors keep their relative order; a surviving vertex's new id is its rank among the surviving vertices and the
 *   faces are re-indexed; index_map[v] = the new id, or -1.  Ranks come from ballots and a scan of block totals, no atomics.
 *
 *   nsr_mesh_components: labels [V] int32 (also the union-find's parent array while the call runs) and *bad_faces.  A lock-free
 *     union-find over the faces that hooks the larger root under the smaller id, then a flatten launch: the root of a component
 *     is its minimum id whatever the interleaving.  No workspace, no host read.
 *   nsr_mesh_component_stats: from labels as nsr_mesh_components left them.  A label outside [0, V) is skipped.
 *   nsr_mesh_filter_count: fills `workspace` (nsr_mesh_filter_workspace_bytes(V, F) bytes, 16-byte aligned: a header
 *     {Vk, Fk, V, F} and the scanned per-block offsets) and writes counts_out[0] = Vk (kept vertices), counts_out[1] = Fk (kept
 *     faces) on the device.  No host read.
 *   nsr_mesh_filter_emit: from the same faces, labels, keep and the workspace the count left: index_map [V], verts_out [Vk,3],
 *     faces_out [Fk,3].  Like nsr_surface_nets_emit it READS THE HEADER BACK ON THE HOST (one stream synchronisation; not legal
 *     inside a stream capture) and refuses a Vk, Fk, V or F that is not the workspace's before anything is launched.
 * V == 0 or F == 0 are legal: no labels or labels[v] = v, Vk = Fk = 0 or the kept singletons; arrays of size 0 may be NULL.
 * NSR_ERR_INVALID_ARG before any launch: V or F >= 2^31 (the workspace size is 0 then), a NULL array of non-zero size, a NULL
 * bad_faces, workspace or counts_out, a pointer not aligned to 4 bytes (workspace: 16; keep: 1), Vk > V, Fk > F, Fk > 0 with
 * Vk == 0, or the mismatch above.
 * ------------------------------------------------------------------------------------------ */
int nsr_mesh_components(const int32_t *faces, uint32_t V, uint32_t F, int32_t *labels, uint32_t *bad_faces, nsr_stream_t stream);
int nsr_mesh_component_stats(const float *verts, const int32_t *faces, const int32_t *labels, uint32_t V, uint32_t F,
                             uint32_t *n_verts, uint32_t *n_faces, float *lo, float *hi, nsr_stream_t stream);
uint64_t nsr_mesh_filter_workspace_bytes(uint32_t V, uint32_t F);
int nsr_mesh_filter_count(const int32_t *faces, const int32_t *labels, const uint8_t *keep, uint32_t V, uint32_t F, void *workspace,
                          uint32_t *counts_out, nsr_stream_t stream);
int nsr_mesh_filter_emit(const float *verts, const int32_t *faces, const int32_t *labels, const uint8_t *keep, uint32_t V,
                         uint32_t F, void *workspace, uint32_t Vk, uint32_t Fk, int32_t *index_map, float *verts_out,
                         int32_t *faces_out, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Occupancy components: connected components of the occupied cells of the occupancy grid, their statistics, and a cull that
 * closes whole components (csrc/occ_components.hip, csrc/occ_cc_core.h; Renderer.cull_floaters).  The volume-level counterpart
 * of the mesh cleaning above: detached specks of density sit in the grid as small islands of occupied cells, and every march
 * walks through them.  Additive: the ABI version stays.  Every output is a pure function of the input: two calls give the same
 * bits.
 *
 * Grid: C cascades of H^3 cells, the shape rule of every nsr_occ_* call (C in 1..8, H a power of two in 8..512, C*H^3 < 2^31).
 * Cell id u = c * H^3 + morton(ix, iy, iz).  Cell u is OCCUPIED iff bit (u & 7) of bitfield byte (u >> 3) is set: the layout
 *   nsr_packbits and nsr_occ_update write and nsr_occ_mark_untrained clears.  Connectivity reads the bitfield only, never
 *   density_grid.
 * Neighbours: two occupied cells of the SAME cascade whose coordinates differ by exactly 1 along exactly one axis
 *   (6-connectivity).  No wrap-around between 0 and H - 1.  No link between cascades: each cascade is labelled, judged and culled
 *   on its own (a link through the coarser cascade, which holds its own full copy of the inner region, would glue any floater
 *   within one coarse cell of the scene back onto it).  Components are the transitive closure.
 * labels [C*H^3] int32: labels[u] = the SMALLEST cell id of u's component if u is occupied, -1 if not.  A root is a u with
 *   labels[u] == u.
 * Statistics, indexed by cell id and meaningful at the roots: n_cells [C*H^3] uint32; lo, hi [C*H^3,3] int32, the inclusive box
 *   of the component in cell coordinates (ix, iy, iz).  A cell that is no root holds 0, lo = H, hi = -1.  Integer adds, mins and
 *   maxes are order-free, so the kernels use atomics and are deterministic all the same.
 * Keep rule (the caller's; nerfstyle_amd/raymarching.py, keep_occupancy_components, elementwise torch on the device with no host
 *   read): a component of cascade c is kept iff n_cells >= min_cells; (2 b_c / H)^2 * (ex^2 + ey^2 + ez^2) >= min_diagonal^2
 *   with e = hi - lo + 1 and b_c = min(2^c, bound), in fp64 in this written order; and, with keep_largest = k, it is among the k
 *   components of the most cells OF ITS OWN CASCADE among those that passed, ties to the smaller label.
 * Cull.  keep [C*H^3] uint8, read at the roots.  For every occupied cell whose component is not kept the bit is cleared and, if
 *   density_grid is given, the cell's word becomes -1.0f (0xBF800000): the untrained state, which nsr_occ_update never leaves and
 *   the occupied-cell list never names (a later nsr_occ_mark_untrained re-opens such a cell if enough cameras see it).  Every
 *   other grid word keeps its bits exactly, NaN and -0.0f included; every other bit stays.  With density_grid NULL only bits are
 *   cleared: the next nsr_occ_update rebuilds them.  n_culled [C] uint32 (optional) is WRITTEN with the cells cleared per cascade
 *   (zeroed by a kernel of the call, then integer atomics of block sums).  A label outside [0, C*H^3) at an occupied cell decides
 *   nothing and is never dereferenced.
 *
 *   nsr_occ_components: an init launch (labels[u] = u or -1), a union launch (a lock-free union-find that hooks the larger root
 *     under the smaller id; a thread owns one bitfield byte, one 2x2x2 Morton block, and unites each of its occupied cells with
 *     its occupied +x, +y, +z neighbours) and a flatten launch.  labels doubles as the parent array while the call runs.
 *   nsr_occ_component_stats: from labels as nsr_occ_components left them.
 *   nsr_occ_cull: bitfield (and density_grid) in place.
 * None of them uses a workspace or reads anything on the host: all three are legal inside a stream capture.
 * NSR_ERR_INVALID_ARG before any launch: the shape rule; a NULL bitfield, labels, keep, n_cells, lo or hi; labels or density_grid
 * not aligned to 16 bytes; n_cells, lo, hi or n_culled not aligned to 4.
 * ------------------------------------------------------------------------------------------ */
int nsr_occ_components(const uint8_t *bitfield, uint32_t C, uint32_t H, int32_t *labels, nsr_stream_t stream);
int nsr_occ_component_stats(const int32_t *labels, uint32_t C, uint32_t H, uint32_t *n_cells, int32_t *lo, int32_t *hi,
                            nsr_stream_t stream);
int nsr_occ_cull(float *density_grid, uint8_t *bitfield, const int32_t *labels, const uint8_t *keep, uint32_t C, uint32_t H,
                 uint32_t *n_culled, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * View reprojection: a rendered frame warped into a neighbouring camera through its depth, and the squared error of the
 * pixels both cameras see (csrc/reproject.hip, csrc/reproject_core.h; nerfstyle_amd/consistency.py).  The warped error between
 * views is the number the stylisation stage is judged by: short range between neighbouring frames, long range between frames
 * several apart.  Additive: the ABI version stays.
 *
 * rgb   [F, H*W, 3] f32, pixel-major rows (the layout of rgb_map).
 * dist  [F, H*W] f32: the distance from the camera origin to the surface along the pixel's unit ray.  "No surface" is any value
 *       that is not finite or not > 0.
 * poses [F, 3, 4] f32 camera to world: R = pose[:, :3], o = pose[:, 3].
 * fx, fy, cx, cy, W, H (both >= 2), camera_flip (0..7): the pinhole of nsr_generate_rays and its flip signs f0, f1, f2 (bits
 *       2, 1, 0 of camera_flip negate axes 0, 1, 2).
 * pairs [P, 2] int32: (dst a, src b).  depth_tol: the relative tolerance of the depth test, >= 0.
 *
 * For pair (a, b) and dst pixel p = py * W + px, everything in fp64 from the f32 inputs, no operation contracted, sums of
 * products added left to right as written:
 *   1. t = dist[a, p]; invalid if it is no surface.
 *   2. c = (((px + 0.5 - cx) / fx) * f0, ((py + 0.5 - cy) / fy) * f1, f2); v = R_a c (v_r = R[r][0] c0 + R[r][1] c1 + R[r][2] c2);
 *      n = sqrt(v0 v0 + v1 v1 + v2 v2); X_r = o_a[r] + t * (v_r / n).
 *   3. dx = X - o_b; q_k = R_b[0][k] dx0 + R_b[1][k] dx1 + R_b[2][k] dx2; z = q2 * f2; invalid unless z > 0.
 *   4. u = fx * (q0 * f0 / z) + cx - 0.5, w = fy * (q1 * f1 / z) + cy - 0.5 (pixel centres at the integers); invalid unless
 *      0 <= u <= W - 1 and 0 <= w <= H - 1.  x0 = min(floor(u), W - 2), y0 = min(floor(w), H - 2), ax = u - x0, ay = w - y0.
 *      The bilinear mean of the taps v00 = [y0, x0], v01 = [y0, x0 + 1], v10 = [y0 + 1, x0], v11 = [y0 + 1, x0 + 1] is
 *      (v00 (1 - ax) + v01 ax) (1 - ay) + (v10 (1 - ax) + v11 ax) ay.
 *   5. All four taps of dist[b] must be a surface, whatever their weights; tbar = their bilinear mean,
 *      r = sqrt(dx0 dx0 + dx1 dx1 + dx2 dx2); invalid (occluded or disoccluded) unless |r - tbar| <= depth_tol * r.
 *   6. warped[p, k] = the bilinear mean of the four taps of rgb[b, :, k], rounded once to f32, and mask[p] = 1.  An invalid
 *      pixel gets warped = 0 and mask = 0.
 *   7. stats[pair] = (sse, n_valid) f64: n_valid the count of valid pixels, sse the sum over them of ((e0 e0 + e1 e1) + e2 e2)
 *      with e_k = warped_k (before its rounding to f32) - rgb[a, p, k].  Summed in fp64 in a fixed order without atomics: per
 *      block of 256 consecutive pixels the block sum of csrc/fixed_sum.h into the block's own slot of the workspace, then the
 *      slots of a pair, thread t of one block taking slots t, t + 256, ... in that order, and the block sum again.  Two calls
 *      give the same bits.
 * A pair that names a frame outside [0, F) reads neither frame: stats = (0, 0), mask 0, warped 0.
 *
 * warped [P, H*W, 3] f32 and mask [P, H*W] uint8 may each be NULL: the metric alone writes stats [P, 2] only.  The outputs must
 * not overlap the inputs.  workspace: nsr_reproject_frames_workspace_bytes(P, H, W) bytes, 8-byte aligned; the query answers 0
 * for a shape the call refuses.  No host read, no allocation: legal inside a stream capture.  P = 0 is a no-op.
 * NSR_ERR_INVALID_ARG before any launch: W < 2 or H < 2, H*W > 2^30, P * ceil(H*W / 256) >= 2^31, F = 0, camera_flip outside
 * 0..7, fx or fy zero or NaN, depth_tol negative or NaN, a NULL rgb, dist, poses, pairs, stats or workspace, a misaligned pointer.
 * ------------------------------------------------------------------------------------------ */
uint64_t nsr_reproject_frames_workspace_bytes(uint32_t P, uint32_t H, uint32_t W);
int nsr_reproject_frames(const float *rgb, const float *dist, const float *poses, uint32_t F, uint32_t H, uint32_t W, float fx, float fy,
                         float cx, float cy, int camera_flip, const int32_t *pairs, uint32_t P, double depth_tol, float *warped,
                         uint8_t *mask, double *stats, void *workspace, nsr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Style image clustering: Lloyd k-means over pixel rows in colour plus weighted position (csrc/kmeans.hip, csrc/km_core.h;
 * nerfstyle_amd/segment.py).  It makes the cluster map of a style image that SemanticStyleLoss(clusters=...) and the region-wise
 * colour transfer above take.  Additive: the ABI version stays.
 *
 * rows: n rows of `stride` f32, stride 3 or 4, read in place, 4-byte aligned (16 with stride 4); the fourth float is never read.
 * H, W >= 1 with n a multiple of H*W (a stack of n / (H*W) frames): row i has x = i % W, y = (i / W) % H.  n <= 2^27.
 * Feature: f = (r, g, b, wxy * x / m, wxy * y / m), m = max(H, W), the position terms formed in fp64 as (wxy * x) / m;
 *   0 <= wxy <= 8, wxy = 0 clusters colour alone.  A row is UNLABELLED (label -1, it contributes to nothing) if any of r, g, b is
 *   NaN, infinite or outside [-8, 8]; so |f_j| <= 8.
 * Assignment: centroids [K][5] fp64 in device memory, 1 <= K <= NSR_COLOR_MAX_REGIONS.  t_j = f_j - c_kj,
 *   d_k = ((((t0 t0 + t1 t1) + t2 t2) + t3 t3) + t4 t4) in fp64, every operation rounded on its own (nothing contracted).  The
 *   label starts as 0 and becomes k, for k = 1 .. K-1 in turn, when d_k < d_label: the smallest distance, the lowest k among
 *   equals.  (Centroids are expected to be finite; a NaN distance never wins that comparison.)
 * Sums are integers: counts[k] = the rows labelled k, sums[k][j] = sum over them of llrint(f_j * 2^32) (exact product, round to
 *   nearest even), both int64.  |sum| <= 2^27 * 2^35 = 2^62.  Integer addition has no order: whichever mix of wave butterflies,
 *   LDS atomics and per-block partials ran, the result is the same, and a NumPy restatement reproduces it exactly.
 * Update: centroids_out[k][j] = (double)sums[k][j] / 4294967296.0 / (double)counts[k]; a cluster with count 0 keeps
 *   centroids[k].  centroids_out may be NULL (no update) or `centroids` itself.
 * stats [2] fp64: stats[0] = the number of rows i with labels[i] != prev_labels[i] (exact; every one of the n rows when prev_labels
 *   is NULL; an unlabelled row that stays unlabelled has not changed), stats[1] = the inertia, the sum of d_label(i) over the
 *   labelled rows, added in fp64 in a fixed order without atomics: per thread in the order of its rows, the block sum of
 *   csrc/fixed_sum.h, one partial per block, then thread t of one block adds partials t, t + 256, ... and the block sum again.  The
 *   order depends on n, stride and, for stride 3, on the rows' offset from a 16-byte boundary, nothing else: two calls give the
 *   same bits.  prev_labels may be `labels` itself (a row's label is read and written by one thread).
 * workspace: the _workspace_bytes query of the same name gives its size in bytes (0 for arguments the call refuses), 8-byte
 *   aligned.  No host read, no allocation: legal inside a stream capture.
 *
 * Maximin init.  Candidates are rows j * s, s = ceil(n / 65536); unlabelled candidates are skipped.  Centre 0 is the candidate
 *   with the smallest d to `mean` [5] (device fp64; segment.py passes the centroid that one step with K = 1 gives: the
 *   fixed-point mean of all labelled rows); centre r the candidate with the largest distance to its nearest centre among 0 .. r-1;
 *   equal distances: the lowest row index; a chosen candidate is not chosen again.  Distances as d above.  centroids [K][5] gets
 *   the chosen rows' features (fp64, not quantised), chosen_rows [K] int32 their row indices, n_labelled [1] uint32 the number of
 *   labelled candidates.  With fewer labelled candidates than K the remaining centres repeat the last one chosen (`mean` if
 *   none) with chosen_rows = -1; the caller reads n_labelled to refuse that case.
 *   workspace: its _workspace_bytes query, 8-byte aligned.  One block; no host read.
 *
 * NSR_ERR_INVALID_ARG before any launch: n = 0 or n > 2^27, stride outside {3, 4}, K = 0 or K > NSR_COLOR_MAX_REGIONS, H or W
 * zero or n not a multiple of H*W, xy_weight outside [0, 8] or NaN, a NULL pointer other than prev_labels and centroids_out, a
 * misaligned pointer.
 * ------------------------------------------------------------------------------------------ */
uint64_t nsr_kmeans_step_workspace_bytes(uint64_t n, uint32_t K);
int nsr_kmeans_step(const float *rows, uint64_t n, uint32_t stride, uint32_t H, uint32_t W, double xy_weight, const double *centroids,
                    uint32_t K, const int32_t *prev_labels, int32_t *labels, int64_t *counts, int64_t *sums, double *centroids_out,
                    double *stats, void *workspace, nsr_stream_t stream);
uint64_t nsr_kmeans_init_workspace_bytes(uint64_t n);
int nsr_kmeans_init(const float *rows, uint64_t n, uint32_t stride, uint32_t H, uint32_t W, double xy_weight, const double *mean,
                    uint32_t K, double *centroids, int32_t *chosen_rows, uint32_t *n_labelled, void *workspace, nsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_H_ */
