/*
 * dcf_hip.h -- C ABI of libdcf_hip.so, the MI355X (gfx950) implementation of the
 * continuous-fusion train-step hot path.
 *
 * The reference (Chanuk-Yang/Deep_Continuous_Fusion_for_Multi-Sensor_3D_Object_Detection)
 * is pure Python on torch: it has no FFI of its own, so the drop-in boundary is the
 * Python module surface (model.py / data_import_carla.py / loss.py / train.py) and THIS
 * header is what that surface binds underneath, through ctypes
 * (deep_continuous_fusion_for_multi-sensor_3d_object_detection_amd/_hip.py).
 * Every entry point names the reference code it replaces (file:line under /root/reference).
 *
 * Conventions:
 *   - plain pointers and sizes; device pointers unless marked HOST; no torch types
 *   - returns 0 on success or a negative DCF_E* code; dcf_last_error() gives the text
 *   - never allocates, frees or synchronises; all work is enqueued on `stream`
 *     (a hipStream_t passed as void*); workspaces are caller-provided
 *   - activations are NHWC ("pixel rows of channels"); dtype DCF_F32, DCF_BF16 or DCF_F16 (IEEE half),
 *     accumulation is always fp32
 *   - counts that are produced on the device (n_valid ...) stay on the device
 */
#ifndef DCF_HIP_H
#define DCF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *dcf_stream_t; /* hipStream_t */

enum { DCF_OK = 0, DCF_EINVAL = -1, DCF_ELAUNCH = -2, DCF_EUNSUPPORTED = -3 };
enum { DCF_F32 = 0, DCF_BF16 = 1, DCF_F16 = 2 };   /* compute / storage type of activations and weight images */
/* COMPAT: the reference's last-writer-wins scatter (data_import_carla.py:236-258), three launches; COMPAT_ROUNDS: the same
 * result by the literal nine rounds (claim pass c, resolve pass c-1), kept as a cross-check; ACCUM: atomic accumulation. */
enum { DCF_VOXEL_COMPAT = 0, DCF_VOXEL_ACCUM = 1, DCF_VOXEL_COMPAT_ROUNDS = 2,
       DCF_VOXEL_OCCUPANCY = 3 /* interpolate=False: voxel of the trunc'd ids := 1 (data_import_carla.py:231-234) */ };
enum { DCF_PROJ_COMPAT = 0, DCF_PROJ_CORRECT = 1 };

const char *dcf_last_error(void);
int dcf_version(void);
/* Tuning options (which kernel / tile shape a launch takes; never the results): each is seeded once per process from the
 * environment variable DCF_<NAME> and changed afterwards only here (value NULL = unset).  Tests use it to compare two
 * kernels on the same input (e.g. "KNN_KERNEL" = "tile" | "wave").  HOST strings. */
int dcf_set_option(const char *name, const char *value);
/* Optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg). */
int dcf_prof_enable(int on);
int dcf_prof_reset(void);
/* Records n empty brackets named "__empty_bracket__": the per-launch cost of the event pair itself. */
int dcf_prof_calibrate(dcf_stream_t stream, int n);
/* Fills up to `cap` records (one per kernel name = template instantiation); `work` receives the summed
 * ALGORITHMIC flops the launches declared (0 for kernels priced in bytes). Returns the number of
 * records. HOST pointers. */
int dcf_prof_read(char *names /*[cap][64]*/, double *total_ms, int64_t *calls, double *work, int cap);
/* Same, plus the algorithmic BYTES the launches declared (0 for launches that declare flops only). */
int dcf_prof_read2(char *names, double *total_ms, int64_t *calls, double *work, double *bytes, int cap);

/* ------------------------------------------------------------------ geometry
 * Replaces CarlaDataset.Voxelization_Projection / Projection
 * (data_import_carla.py:196-267, constants :31-43).                          */

/* Range filter + order-preserving compaction (data_import_carla.py:215-229).
 * lim HOST float[6] = {xlo,xhi,ylo,yhi,zlo,zhi}, strict inequalities.
 * out_pts [n][3], out_src [n] (may be NULL), count_dev int[1].
 * ws: dcf_compact_workspace_bytes(n). */
size_t dcf_compact_workspace_bytes(int n);
int dcf_range_filter(const float *pts, int n, const float *lim, float *out_pts, int32_t *out_src,
                     int32_t *count_dev, void *ws, dcf_stream_t stream);

/* Trilinear voxeliser (data_import_carla.py:236-258). Raw points in, range filter fused.
 * aff HOST float[6] = {sx,ox,sy,oy,sz,oz}.  grid [Cz][L][W] fp32 is fully written.
 * mode COMPAT: bit-exact "last writer wins per corner pass" (SURVEY.md F3);
 *      ACCUM : atomic trilinear splat.
 *      COMPAT_ROUNDS: the same grid by the literal nine rounds;  OCCUPANCY: the point's cell is set to 1.
 * owner_ws: int32[2][Cz*L*W], must be ZERO on entry and is returned ZERO (COMPAT, COMPAT_ROUNDS only).
 * Corners and the grid's end.  Indices are FLAT, v = (z*L + x)*W + y, as in the reference: a corner one past the end of a row
 * is the first voxel of the next row and is kept.  In every mode, and in the batch entries below, a corner whose flat index
 * lies outside [0, Cz*L*W) contributes nothing and is never used as an address -- of the grid or of owner_ws.  Limits that
 * leave less than a cell of margin reach such corners (32x64x32, aff 4,0,4,16,10,24: the last two floats below z = 0.6f have
 * fz == 30.0, and with xl == 63 the corners (zl+1, xl+1, .) lie past the last voxel); that is legal.
 * Refused with DCF_EINVAL, nothing launched, nothing written: a non-finite lim or aff; limits under which the LOWER corner
 * (the point's own cell) can leave [0, Cz*L*W) -- judged with the kernels' chain fl(fl(p*s)+o) at the first float above
 * each lower limit and the last float below each upper limit (both ends per axis, so a negative scale is handled). */
size_t dcf_voxelize_workspace_bytes(int Cz, int L, int W);
int dcf_voxelize(const float *pts, int n, const float *lim, const float *aff, int Cz, int L, int W,
                 int mode, float *grid, void *owner_ws, dcf_stream_t stream);
/* Compat-mode voxeliser for the B frames of a batch (claim / gather / release, one launch each for all frames).  pts / n: HOST arrays of B device pointers / point counts; grids [B][Cz][L][W];
 * owner_ws: B * dcf_voxelize_workspace_bytes(Cz,L,W), zero on entry, returned zero.  Same results as B dcf_voxelize calls. */
#define DCF_MAX_VOXEL_BATCH 8
int dcf_voxelize_batch(const float *const *pts, const int *n, int B, const float *lim, const float *aff, int Cz, int L, int W,
                       float *grids, void *owner_ws, dcf_stream_t stream);
/* Same grids written as the engine's input image: x_nhwc [B][L][W][Cz] in `dtype` (what dcf_nchw_to_nhwc makes of the fp32
 * grids, bit for bit: a voxel's value is produced in one piece and rounded once).  Saves the fp32 grid and its transpose. */
int dcf_voxelize_batch_nhwc(int dtype, const float *const *pts, const int *n, int B, const float *lim, const float *aff, int Cz, int L,
                            int W, void *x_nhwc, void *owner_ws, dcf_stream_t stream);

/* Pinhole projection + in-image filter + compaction (data_import_carla.py:196-210,:261-266).
 * Raw points in; keeps points passing the range filter AND the image test, in order.
 * crt HOST float[12] = CRT_tensor [4][3].  uv_out [n][2], xyz_out [n][3], src_out [n] or NULL.
 * Rows >= *count_dev are left untouched (caller pre-zeroes for the zero padding of :263-266). */
int dcf_project_filter(const float *pts, int n, const float *lim, const float *crt, float ulim, float vlim,
                       int mode, float *uv_out, float *xyz_out, int32_t *src_out, int32_t *count_dev,
                       void *ws, dcf_stream_t stream);
/* The same for the B (<= 8) frames of a batch in one launch per phase (count / scan / scatter), every frame with its own points,
 * count and matrix: pts / n HOST arrays of B device pointers / point counts, crt HOST float[B][12]; uv_out [B][rows][2], xyz_out
 * [B][rows][3] (rows >= every n[b]), count_dev [B]; ws: B * dcf_compact_workspace_bytes(max n).  Bit-identical to B calls. */
int dcf_project_filter_batch(const float *const *pts, const int *n, int B, const float *lim, const float *crt, float ulim, float vlim,
                             int mode, float *uv_out, float *xyz_out, int rows, int32_t *count_dev, void *ws, dcf_stream_t stream);

/* The camera visibility mask for the B (<= 8) frames of a batch in one launch (host statement: visibility.py).
 * HOST arrays: pts / out B device pointers to [n[b]][3] points (4-byte alignment is all that is assumed; out[b] == pts[b] is
 * allowed, any other overlap is refused), n B row counts (0 is legal), crt float[B][12] one projection matrix per frame, m B occluder
 * counts (<= 16), occ float[B][16][5] = {x0, y0, x1, y1, D} (finite, x1 >= x0, y1 >= y0: refused otherwise; may be NULL when every
 * m[b] is 0); lim float[6], ulim, vlim, mode as in dcf_project_filter.  With (u, v, a2) the projection's own fp32 chain
 *   a_j = fma(1, c[3][j], fma(z, c[2][j], fma(y, c[1][j], fl(x c[0][j]))))   u = fl(a0 / a2)   v = fl(a1 / a2)
 * row i of frame b is written as (+inf, +inf, +inf) iff
 *   (fov != 0 and the row fails dcf_project_filter's keep predicate) or
 *   (for some occluder j < m[b]:  u >= x0 && u < x1 && v >= y0 && v < y1 && a2 > D)        (a NaN compares false)
 * and is copied bit for bit otherwise (a NaN keeps its payload).  Every range test of this library rejects a +inf row: nothing is
 * compacted, the point counts do not change.  Nothing is written beyond row n[b].  The tables travel in the kernel argument. */
int dcf_camera_mask_points_batch(const float *const *pts, const int *n, int B, const float *lim, const float *crt, float ulim, float vlim,
                                 int mode, int fov, const int *m, const float *occ, float *const *out, dcf_stream_t stream);

/* Train-time BEV augmentation of the B (<= 8) frames of a batch in one launch (host statement: augment.py).
 * pts / out: HOST arrays of B device pointers to [n[b]][3] points (4-byte alignment is all that is assumed; out[b] == pts[b] is
 * allowed, any other overlap is refused); n HOST int[B] (0 is legal); mat HOST float[B][5] = {a00, a01, a10, a11, a22} of
 * A = s R(theta) diag(1, f, 1) rounded once to fp32; drop_key HOST uint64[B], drop_thresh HOST uint32[B].
 *   x' = fl(fl(a00 x) + fl(a01 y))   y' = fl(fl(a10 x) + fl(a11 y))   z' = fl(a22 z)          (no contraction)
 * Point i of frame b is dropped iff (mix64(drop_key[b] ^ mix64(i)) >> 32) < drop_thresh[b] (mix64: the finaliser of the loss
 * sampler's hash) and is then written as (+inf, +inf, +inf), which every range test of this library rejects: nothing is
 * compacted, the point counts do not change. */
int dcf_augment_points_batch(const float *const *pts, const int *n, int B, const float *mat, const uint64_t *drop_key,
                             const uint32_t *drop_thresh, float *const *out, dcf_stream_t stream);

/* Train-time camera image augmentation of the B (<= 8) frames of a batch in one launch (host statement:
 * augment_image.py).  img / out: device uint8 [B][3][H][W], contiguous, ANY byte alignment (a view into a larger buffer is fine),
 * 3 H W <= 2^30; out must not overlap img (the kernel gathers neighbours; refused).  q HOST float[B][8] = {ku, cu, kv, cv, g0,
 * g1, g2, bias}, finite: the inverse of the image-plane affine u' = u / ku - cu / ku (likewise v) and the photometric line, each
 * rounded once to fp32.  For the output pixel (h, w), every operation rounded to fp32, nothing contracted:
 *   fx = ((ku (w + .5)) + cu) - .5   x0 = floor(fx)   wx = fx - x0        (fy, y0, wy from h, kv, cv)
 *   top = p00 (1 - wx) + p01 wx   bot likewise   val = top (1 - wy) + bot wy   t = g_c val + bias
 *   out = clamp(rint(t), 0, 255), round half to even; a tap outside the image contributes 0. */
int dcf_augment_image_batch(const uint8_t *img, int B, int H, int W, const float *q, uint8_t *out, dcf_stream_t stream);

/* Train-time object pasting, the points (host statement: paste.py) for the B (<= 8) frames of a batch in one
 * launch.  HOST arrays: pts / out B device pointers (4-byte aligned), n B row counts, m B record counts (<= 16), rec float[B][16][8] =
 * {cx, cy, cz, cos yaw, sin yaw, l/2 + margin, w/2 + margin, h/2 + margin} (rounded once from float64), app int64[B][16][2] =
 * (first bank row, rows) of the pasted objects, out_rows B output capacities in rows.  bank: device fp32 [bank_rows][3].
 * Frame b, a_b = the sum of its objects' rows: output row i < n_b is the source row bit for bit, or (+inf, +inf, +inf) when,
 * for any record, every operation rounded to fp32 and nothing contracted,
 *   dx = x - cx   dy = y - cy   lx = dx c + dy s   ly = dy c - dx s   |lx| <= hl && |ly| <= hw && |z - cz| <= hh
 * (NaN / infinite coordinates compare false); row n_b + prefix_j + i is bank row start_j + i; nothing is written beyond row
 * n_b + a_b (<= out_rows[b], refused otherwise).  An output overlaps no input, no other output and not the bank (refused).
 * The per-frame tables: up to 4 frames they travel in the kernel argument and the staging pointers may be NULL.  5 .. 8 frames
 * need stage_host / stage_dev: stage_bytes >= 8192 of PINNED host memory and of device memory, 8-byte aligned: the call packs its
 * table into stage_host and enqueues ONE copy to stage_dev in front of the launch, on `stream`; both stay untouched until the
 * stream has passed the launch (the caller keeps a ring).  The host never waits. */
int dcf_paste_points_batch(const float *const *pts, const int *n, int B, const int *m, const float *rec, const int64_t *app,
                           const float *bank, int64_t bank_rows, float *const *out, const int *out_rows, void *stage_host,
                           void *stage_dev, size_t stage_bytes, dcf_stream_t stream);

/* Train-time object pasting, the image patches, for the B (<= 8) frames of a batch in one launch.  img / out: device uint8
 * [B][3][H][W], contiguous, ANY byte alignment, 3 H W <= 2^30, not overlapping (refused).  HOST arrays: m B record counts (<= 16),
 * rec int64[B][16][9] = {x0, y0, w, h, sx, sy, pw, ph, start}: the destination rectangle inside the image, the offset of its first
 * pixel inside the patch, the patch's width and height, and the first byte of the patch [3][ph][pw] in bank (device uint8
 * [bank_bytes]); every index is checked on the host.  Output byte (c, y, x) = bank[start + (c ph + (y - y0 + sy)) pw + (x - x0 + sx)]
 * of the LAST listed record whose rectangle contains (x, y), the input byte where none does: a function of the output pixel
 * alone, no atomics, no dependence on launch order.  stage_host / stage_dev as in dcf_paste_points_batch. */
int dcf_paste_patches_batch(const uint8_t *img, int B, int H, int W, const int *m, const int64_t *rec, const uint8_t *bank,
                            int64_t bank_bytes, uint8_t *out, void *stage_host, void *stage_dev, size_t stage_bytes, dcf_stream_t stream);

/* BEV K-nearest-neighbour (reference: model.py:199-203 TODO; spec SURVEY.md App. D).
 * xyz [n_max][3], first *count_dev rows valid.  idx_out int32 [K][h][w], -1 padding.
 * rmax2 < 0 = unbounded.  K <= 8.  ws: dcf_knn_workspace_bytes(n_max,h,w).
 * Order: ascending (d2, index), d2 = fl(fl(dx dx) + fl(dy dy)) to the pixel centre; d2 == rmax2 is kept.  A point outside
 * the site is sorted into the nearest border cell and takes part with its true distance.  The valid rows are FINITE by
 * construction -- they are what dcf_project_filter kept, and its range test rejects NaN and infinite coordinates; the
 * result for a non-finite valid row is not defined (rows past *count_dev may hold anything). */
size_t dcf_knn_workspace_bytes(int n_max, int h, int w);
int dcf_knn_bev(const float *xyz, const int32_t *count_dev, int n_max, int K, int h, int w, int stride,
                float xs, float xo, float ys, float yo, float rmax2, int32_t *idx_out, void *ws,
                dcf_stream_t stream);
/* The B frames of a batch in one launch per phase: xyz [B][n_max][3], count_dev [B], idx_out [B][K][h][w]; ws = B workspaces of
 * dcf_knn_workspace_bytes(n_max, h, w), ws_stride_bytes apart (a multiple of 16).  Same indices as B calls of dcf_knn_bev. */
int dcf_knn_bev_batch(const float *xyz, const int32_t *count_dev, int B, int n_max, int K, int h, int w, int stride,
                      float xs, float xo, float ys, float yo, float rmax2, int32_t *idx_out, void *ws, size_t ws_stride_bytes,
                      dcf_stream_t stream);

/* A coarser site of the same batch (stride a multiple of fine_stride): its own cell sort as dcf_knn_bev_batch (ws), and a search
 * that serves the pixels of dense regions from the cells a FINER site's dcf_knn_bev_batch call has already built (ws_fine = that
 * call's workspace, untouched since; same xyz / count_dev / n_max / B) -- a few dozen candidates per pixel instead of the
 * hundreds to thousands a coarse cell window holds near the sensor.  Same indices as dcf_knn_bev_batch. */
int dcf_knn_bev_batch_shared(const float *xyz, const int32_t *count_dev, int B, int n_max, int K, int h, int w, int stride,
                             int fine_h, int fine_w, int fine_stride, float xs, float xo, float ys, float yo, float rmax2,
                             int32_t *idx_out, void *ws, size_t ws_stride_bytes, const void *ws_fine, size_t ws_fine_stride_bytes,
                             dcf_stream_t stream);

/* All fusion sites of a batch in one call: the cell sort of every site in one launch per phase, then each site's search as
 * dcf_knn_bev_batch (fine = -1) or dcf_knn_bev_batch_shared (fine = index of an earlier, finer site of the call) runs it: the
 * same maps bit for bit, 6 sort launches instead of 6 per site.  The reference computes these indices once per frame in its
 * loader (data_import_carla.py: the commented KNN block).  sites is a HOST array of 1..4 entries; every ws is
 * 16-byte aligned with frames ws_stride_bytes apart (>= dcf_knn_workspace_bytes(n_max, h, w), multiple of 16). */
typedef struct { int32_t h, w, stride, fine; int32_t *idx_out; void *ws; size_t ws_stride_bytes; } dcf_knn_site;
int dcf_knn_bev_sites(const float *xyz, const int32_t *count_dev, int B, int n_max, int K, const dcf_knn_site *sites, int nsites,
                      float xs, float xo, float ys, float yo, float rmax2, dcf_stream_t stream);

/* Inverse of the KNN maps of a step (sites x frames) for the fusion backward: the (pixel, point) pairs of every
 * idx [K][h][w] counting-sorted by (map, point).  start int32 [nmaps*(n_max+1)]: pairs of point q of map g are
 * [start[g*(n_max+1)+q], start[g*(n_max+1)+q+1]); ent_pix / ent_pt int32 [sum K*h*w] (pixel packed (i<<16)|j).
 * maps is a HOST array.  ws: dcf_fusion_invert_workspace_bytes(n_max, nmaps).  Pair order inside a point is not
 * deterministic (atomic cursor). */
#define DCF_MAX_KNN_MAPS 32
typedef struct { const int32_t *idx; int32_t h, w; } dcf_knn_map;
size_t dcf_fusion_invert_workspace_bytes(int n_max, int nmaps);
int dcf_fusion_invert(const dcf_knn_map *maps, int nmaps, int K, int n_max, int32_t *start, int32_t *ent_pix, int32_t *ent_pt,
                      void *ws, dcf_stream_t stream);

/* ------------------------------------------------------------ layout / input
 * NCHW fp32 -> NHWC dtype (the model keeps the reference's NCHW voxel input, model.py:194). */
int dcf_nchw_to_nhwc(int dtype, const float *x, void *y, int B, int C, int H, int W, dcf_stream_t stream);
/* NHWC dtype -> NCHW fp32: stage outputs handed back in the reference's layout (model.py:76-79). */
int dcf_nhwc_to_nchw(int dtype, const void *x, float *y, int B, int C, int H, int W, dcf_stream_t stream);
/* uint8 NCHW image -> x/255 as NHWC with C padded to 4 and a zero halo of 3 pixels (stem input). */
int dcf_image_to_nhwc4(int dtype, const uint8_t *img, void *y, int B, int H, int W, dcf_stream_t stream);
/* (version 202 still: an addition) The same with the input normalisation of `fusion.image_norm`: per plane c
 * of the input's own order and byte s,  v = fl(fl(fl((float)s / 255) - mean[c]) / std[c])  -- three correctly rounded fp32
 * operations, nothing contracted, no reciprocal.  Halo pixels and channel 3 are +0.  mean, std: HOST float[3], copied into the kernel
 * argument; mean finite, std finite and > 0.  With mean = 0 and std = 1 every stored bit is dcf_image_to_nhwc4's. */
int dcf_image_to_nhwc4_norm(int dtype, const uint8_t *img, void *y, int B, int H, int W, const float *mean, const float *std,
                            dcf_stream_t stream);

/* -------------------------------------------------------------- convolution
 * Replaces nn.Conv2d (+ folded eval BatchNorm + residual + ReLU) of model.py:15-41,147-157.
 * Implicit GEMM on MFMA; x [B,H,W,Cin], w [Cout][kh][kw][Cin] (dtype), y [B,Ho,Wo,Cout].
 * y = act(conv(x,w) + shift[c] + res);  shift fp32 [Cout] or NULL; res (dtype, like y) or NULL.
 * Cin*esize must be a multiple of 64 bytes; Cout a multiple of 32.
 * Every tensor of the convolution entries below (activations, weights, shift, residuals, masks, slabs, gsum) must be 16-byte
 * aligned -- the kernels move 16 bytes per access -- and needs no more than that (tests/test_gpu_conv_exact.py writes every
 * output 16 bytes past a 32-byte boundary). */
int dcf_conv2d_fwd(int dtype, const void *x, const void *w, const float *shift, const void *res, void *y,
                   int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                   int relu, dcf_stream_t stream);
/* 1x1 layers: the shift scaled per output pixel, y = act(conv(x,w) + rowscale[m]*shift[c] + res); rowscale fp32 [B*Ho*Wo].
 * The bias of the fusion site's second Linear layer under the neighbour sum (reference model.py:216-219:
 * sum_k (W2 h_k + b2) = W2 sum_k h_k + cnt*b2), in the GEMM's epilogue. */
int dcf_conv2d_fwd_rowscale(int dtype, const void *x, const void *w, const float *shift, const float *rowscale, const void *res,
                            void *y, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                            int relu, dcf_stream_t stream);
/* Input gradient: gx [B,H,W,Cin] = conv_transpose(gy [B,Ho,Wo,Cout], wt) (+ res).
 * wt [Cin][kh][kw][Cout] (dtype) as produced by dcf_weight_prep.
 * Optional fused ReLU backward of the layer that produced x: mask (dtype, like gx) zeroes gx where
 * mask <= 0. */
int dcf_conv2d_dgrad(int dtype, const void *gy, const void *wt, const void *res, const void *mask, void *gx,
                     int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                     dcf_stream_t stream);
/* The same for a stride-2 layer with a kernel wider than 1x1, plus a residual that lives on the (2i, 2j)
 * sub-grid of gx: resq [B,ceil(H/2),ceil(W/2),Cin] (dtype).  gx = (dgrad + res + scatter(resq)) * (mask > 0).
 * resq is the input gradient of the block's 1x1 / stride-2 shortcut (reference model.py:27-30, 38-40),
 * computed on its own grid by dcf_conv2d_dgrad(..., H = ceil(H/2), W = ceil(W/2), stride = 1). */
int dcf_conv2d_dgrad_halfres(int dtype, const void *gy, const void *wt, const void *res, const void *resq,
                             const void *mask, void *gx, int B, int H, int W, int Cin, int Ho, int Wo, int Cout,
                             int kh, int kw, int stride, int pad, dcf_stream_t stream);
/* Several INDEPENDENT forward convolutions / input gradients in one call (HOST arrays; no item may read or overwrite what another
 * item writes).  Items that the generic implicit-GEMM kernel would run with the same instantiation (dtype, K chunk, tile) share
 * one launch, up to 4 layers each: every layer keeps its own workgroups and its own arithmetic, so each result is bit for bit
 * what dcf_conv2d_fwd / dcf_conv2d_dgrad write; what is saved is the kernel boundary between small launches.  Everything else
 * -- fp32, 3x3 / stride-1 layers (they have kernels of their own), stride-2 input gradients, a bucket of one, an instantiation
 * without a grouped form -- goes through the single-layer entry points inside the call.  Option "IGEMM_GROUP" = "0": every item
 * takes its single-layer launch.  Fields as the arguments of dcf_conv2d_fwd / dcf_conv2d_dgrad. */
typedef struct {
    int32_t dtype, relu;
    const void *x, *w;
    const float *shift;        /* may be NULL */
    const void *res;           /* may be NULL */
    void *y;
    int32_t B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, pad_;
} dcf_conv_fwd_item;
typedef struct {
    int32_t dtype, pad_;
    const void *gy, *wt;
    const void *res, *mask;    /* may be NULL */
    void *gx;
    int32_t B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, pad2_;
} dcf_conv_dgrad_item;
int dcf_conv2d_fwd_group(const dcf_conv_fwd_item *items, int n, dcf_stream_t stream);
int dcf_conv2d_dgrad_group(const dcf_conv_dgrad_item *items, int n, dcf_stream_t stream);
/* ---- A CHAIN of 3x3 / stride-1 / pad-1 layers with C channels in and out, each reading the one before it, in ONE launch
 * (csrc/conv_rs.hip, chain mode): the bodies of a residual stage -- /root/reference/model.py:32-41, conv1 -> bn1 -> relu ->
 * conv2 -> bn2 -> += shortcut -> relu, block after block (model.py:48-60) -- forward, or (flip = 1, weights = the
 * [Cin][tap][Cout] images) the same list backwards for the input gradients.  Layer l computes exactly what
 *   dcf_conv2d_fwd(dtype, x, w, shift, res, y, B, H, W, C, H, W, C, 3, 3, 1, 1, relu)            (flip = 0)
 *   dcf_conv2d_dgrad(dtype, x, w, res, mask, y, B, H, W, C, H, W, C, 3, 3, 1, 1)                 (flip = 1; shift / relu unused)
 * computes with its row-sharing kernel -- bit-identical results -- but a workgroup moves from its tile of layer l to its tile of
 * layer l + 1 as soon as the neighbouring tiles of layer l are complete (per-tile arrival counters, write-through stores, sc1
 * loads: no kernel boundary, no grid-wide wait).  layers is a HOST array; layers[l].x must be layers[l - 1].y; res may be
 * any tensor written before the launch or the y of a layer at least two back; outputs must be distinct tensors.
 * ws: dcf_conv3x3_chain_workspace_bytes(...) bytes, ZEROED ONCE by the caller when allocated (the launch leaves it zero);
 * one workspace per stream of launches.  dcf_conv3x3_chain_supported: 16-bit dtypes, C % 64 == 0, a layer's tiles fit one
 * round of workgroups (option CONV_CHAIN=0 answers no).  A workgroup whose bounded wait expires writes a record to
 * ((int32_t *)ws)[1] (0 = none; 0x40000000 | layer << 16 | position tile) and stops waiting: results are then wrong, the GPU
 * is not hung; callers that want to know copy that word back (tests do after every launch). */
#define DCF_CHAIN_MAX_LAYERS 24
typedef struct {
    const void *x, *w;
    const float *shift;        /* fp32 [C] or NULL */
    const void *res, *mask;    /* dtype [B,H,W,C] or NULL */
    void *y;
    int32_t relu, pad_;
} dcf_chain_layer;
int dcf_conv3x3_chain_supported(int dtype, int B, int H, int W, int C, int nlayers);
size_t dcf_conv3x3_chain_workspace_bytes(int dtype, int B, int H, int W, int C, int nlayers);
int dcf_conv3x3_chain(int dtype, const dcf_chain_layer *layers, int nlayers, int B, int H, int W, int C, int flip,
                      void *ws, dcf_stream_t stream);
/* Weight gradient, split over pixel ranges: slabs fp32 [nsplit][Cout][kh][kw][Cin] (plain stores,
 * reduced in fixed order by dcf_wgrad_finalize => bitwise reproducible).
 * gsum (optional) fp32 [4*nsplit][Cout]: per-wave sums over pixels of gy (dL/dbeta of a folded BN),
 * accumulated by the same kernel from the gy fragments it already holds.
 * nsplit = dcf_conv2d_wgrad_splits(...). */
int dcf_conv2d_wgrad_splits(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride);
int dcf_conv2d_wgrad(int dtype, const void *x, const void *gy, float *slabs, float *gsum, int nsplit,
                     int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                     dcf_stream_t stream);
/* The weight gradients of a backward pass are independent of each other: dcf_conv2d_wgrad_group takes all of them (a
 * HOST array) and issues them kernel class by kernel class, up to 32 layers per launch -- the next layer's workgroups
 * start as the previous one's finish (no drain / launch bubble, no idle tail).  Layers of the LDS-DMA row-sharing kernel
 * (dcf_conv2d_wgrad_groupable() == 1: 3x3 / stride 1 / pad 1, 16-bit dtype, >= 64 channels on both sides) and of the
 * generic kernel are grouped; the remaining ones (fp32, 32-channel row-sharing layers) are launched one by one.
 * x / gy must stay alive and unmodified until the call.  Same slabs / gsum / nsplit as dcf_conv2d_wgrad. */
typedef struct {
    int32_t dtype, nsplit;
    const void *x, *gy;
    float *slabs, *gsum;       /* gsum may be NULL */
    int32_t B, H, W, Cin, Cout, kh, kw, stride, pad, pad_;
} dcf_wgrad_item;
int dcf_conv2d_wgrad_groupable(int dtype, int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad);
int dcf_conv2d_wgrad_group(const dcf_wgrad_item *items, int n, dcf_stream_t stream);
/* The 7x7/2 RGB stem of the image stream on the NHWC4+halo image. */
int dcf_stem7x7_fwd(int dtype, const void *img4, const void *w, const float *shift, void *y,
                    int B, int H, int W, int Ho, int Wo, int Cout, int relu, dcf_stream_t stream);
int dcf_stem7x7_wgrad(int dtype, const void *img4, const void *gy, float *slabs, float *gsum, int nsplit,
                      int B, int H, int W, int Ho, int Wo, int Cout, dcf_stream_t stream);

/* Per-step parameter preparation (table driven, one launch for the whole net):
 * for conv i: scale = gamma*rsqrt(var+eps) (or 1), shift = beta - mean*scale (or 0),
 * w_fwd = cast(scale[co]*W), w_dgrad = transpose of the same.  Descriptor table lives on
 * the device (struct dcf_conv_param, below).  cin and cout_pad must be multiples of 32.
 * What the kernels rely on without checking it (they load and store 16 bytes per lane):
 *   - w_off is a multiple of 4 elements (and so is every row, K = taps*cin being a multiple of 32);
 *   - wfwd_off, wdgrad_off and w8_off (dcf_f8_param) are 16-byte aligned -- the product rounds them to 256 bytes;
 *   - slab_off is a multiple of 4 elements;
 *   - a range a layer owns in one arena overlaps no other layer's: the kernels write rows co < cout_pad of the weight
 *     images, scale / shift and wscale (zeros for co >= cout) and rows co < cout of the gradients, nothing else.
 * (pinned by tests/test_gpu_prep_finalize.py against the fp64 statements of tests/_prep_ref.py) */
typedef struct dcf_conv_param {
    int64_t w_off;      /* element offset of W [Cout][taps][Cin] fp32 in the parameter arena */
    int64_t gamma_off;  /* BN gamma/beta offsets in the parameter arena, -1 = no BN            */
    int64_t beta_off;
    int64_t mean_off;   /* running mean/var offsets in the buffer arena                        */
    int64_t var_off;
    int64_t wfwd_off;   /* byte offsets into the compute-dtype weight arena                    */
    int64_t wdgrad_off; /* -1 = not needed                                                      */
    int64_t shift_off;  /* element offset into the fp32 scale/shift arena: [scale Cout][shift Cout] */
    int64_t slab_off;   /* element offset of this conv's wgrad slabs in the slab arena         */
    int64_t gsum_off;   /* element offset of this conv's [4*nsplit][cout_pad] sums of g in the gsum arena */
    int32_t cout, cin, taps, cout_pad;
    int32_t nsplit, flags, pad0, pad1;
} dcf_conv_param;
int dcf_weight_prep(int dtype, const dcf_conv_param *table, int nconv, const float *params, const float *buffers,
                    void *warena, float *ssarena, float eps, dcf_stream_t stream);
/* Reduce wgrad slabs in split order and apply the folded-BN chain rule:
 * dW = scale*G, dgamma = (<W,G> - mean*dbeta)*invstd, dbeta = sum over the 4*nsplit rows of gsum[.][co]. */
/* max_cout = the largest cout of the table (grid width): a layer whose cout exceeds it keeps rows max_cout .. cout - 1
 * of its gradients UNFINALISED (no workgroup exists for them, no error is raised). */
int dcf_wgrad_finalize(const dcf_conv_param *table, int nconv, int max_cout, const float *params, const float *buffers,
                       const float *ssarena, const float *slabs, const float *gsum, float *grads, float eps,
                       dcf_stream_t stream);
/* Same, with the layers' cout values on the HOST (cout_host[nconv], nconv <= 256): one workgroup per (conv, output channel)
 * exactly, instead of a max_cout x nconv grid whose surplus workgroups exit at once.  Above 256 layers the call is
 * still valid: it launches the grid form with max_cout = max(cout_host) -- same bits, no error. */
int dcf_wgrad_finalize_rows(const dcf_conv_param *table, int nconv, const int32_t *cout_host, const float *params, const float *buffers,
                            const float *ssarena, const float *slabs, const float *gsum, float *grads, float eps,
                            dcf_stream_t stream);

/* ------------------------------------------------------------- fp8 forward convolutions (csrc/conv_fp8.hip)
 * BASELINE.json configs[4] / SURVEY.md 8(d) cfg5 ("fp8 MFMA convs, fp32 accumulate, bf16 epilogue"); the reference has
 * no counterpart (model.py runs fp32 nn.Conv2d, model.py:16-19).  Operands are OCP e4m3 on
 * v_mfma_scale_f32_32x32x64_f8f6f4; weights carry one scale per output channel, activations one power-of-two scale per
 * tensor derived on the device from the tensor's absolute maximum one step earlier (delayed scaling, no host sync):
 *   y = act((sum_k q(x*sx) q(w*sw[co])) / (sx*sw[co]) + shift[co] + res)
 * dcf_fp8_act_scale: the scale rule -- the largest power of two s <= 2^126 with amax*s <= 224 for every positive finite
 * amax (subnormals and FLT_MAX included), 1 when amax is zero, negative, Inf or NaN.  The cap keeps the scale finite for
 * amax < 224 / FLT_MAX and 1/s a normal number.  Host and kernels derive the same bits.
 * q(): round to nearest even on the e4m3 grid after saturation: |v| > 448 and +-Inf become +-448; NaN stays NaN (either
 * e4m3 NaN code) in dcf_cast_fp8 and in the y8 image of dcf_conv2d_fwd_fp8 alike, and a NaN operand makes every output
 * whose window covers it NaN (a ReLU epilogue is max(v, 0) as in the 16-bit kernels and returns 0 for it).
 * Recorded maxima (amax_cur, y8cur) are the largest FINITE magnitude: Inf and NaN elements are left out one by one. */
int dcf_fp8_act_scale(float amax, float *scale);
/* x8[i] = q(x[i] * dcf_fp8_act_scale(*amax_prev)) (amax_prev null: scale 1).  amax_cur (optional): 64 device floats
 * holding partial maxima of the finite |x| -- each workgroup raises one of them (never lowers it), so the tensor's maximum
 * is the max over the 64 (one hot address would serialise the atomics).  n multiple of 8. */
int dcf_cast_fp8(int dtype, const void *x, void *x8, const float *amax_prev, float *amax_cur, int64_t n, dcf_stream_t stream);
/* Per-conv fp8 weight images: w8 [cout_pad][taps][cin] = q(bn_scale*W * 448/amax_co) at byte offset w8_off of w8arena,
 * dequantisation factors amax_co/448 at element offset wscale_off of wsarena (w8_off < 0: conv not on the fp8 path:
 * nothing of it is touched, its amax block included).  An all-zero row gets zero bits and the factor 1, rows
 * co >= cout zero bits and the factor 0.
 * Also rolls each conv's activation maxima: amax holds DCF_F8_AMAX_STRIDE floats per conv, [0..63] the partial maxima of
 * the current step and [64] the previous step's maximum (the scale source): prev <- max(cur[0..63]), cur <- 0. */
#define DCF_F8_AMAX_STRIDE 80
typedef struct dcf_f8_param {
    int64_t w8_off;
    int64_t wscale_off;
} dcf_f8_param;
int dcf_weight_prep_fp8(const dcf_conv_param *table, const dcf_f8_param *f8table, int nconv, int max_cout_pad, const float *params,
                        const float *buffers, void *w8arena, float *wsarena, float *amax, float eps, dcf_stream_t stream);
/* Forward convolution over fp8 images: x8 [B][H][W][Cin], w8 [Cout][kh][kw][Cin], wscale [Cout], xamax = the device
 * scalar dcf_cast_fp8 derived x8's scale from (null: 1); shift / res / relu as dcf_conv2d_fwd; y, res in out_dtype.
 * Optional second output for the convolution that consumes y: y8 = dcf_cast_fp8(y) with the scale of *y8amax, partial
 * maxima of |y| raised in y8cur[64] (either may be null).  Cin multiple of 64, Cout multiple of 32. */
int dcf_conv2d_fwd_fp8(int out_dtype, const void *x8, const void *w8, const float *wscale, const float *xamax, const float *shift,
                       const void *res, void *y, void *y8, const float *y8amax, float *y8cur, int B, int H, int W, int Cin,
                       int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int relu, dcf_stream_t stream);

/* ------------------------------------------------------------- elementwise
 * g = gy * (y > 0) in place on gy (ReLU backward, model.py:21,25) and per-channel sums
 * gsum[c] += sum_p g[p][c] (the BN-beta gradient).  gsum fp32 [C], pre-zeroed by caller. */
int dcf_relu_bwd_chansum(int dtype, void *gy, const void *y, float *gsum, int64_t npix, int C, int relu,
                         dcf_stream_t stream);
/* Bilinear resize NHWC (model.py:149,151 nn.UpsamplingBilinear2d => align_corners=1; the
 * image FPN uses align_corners=0).  y = resize(x) + (add ? add : 0). */
int dcf_resize_bilinear_fwd(int dtype, const void *x, const void *add, void *y, int B, int Hi, int Wi, int Ho, int Wo,
                            int C, int align_corners, dcf_stream_t stream);
/* gx = resize^T(gy): gather form (each input pixel sums its contributing output pixels). */
int dcf_resize_bilinear_bwd(int dtype, const void *gy, void *gx, int B, int Hi, int Wi, int Ho, int Wo, int C,
                            int align_corners, dcf_stream_t stream);
/* 3x3/2 max-pool pad 1 (image stem), NHWC; bwd routes to the first arg-max in scan order.  Every entry, forward and
 * backward, requires Ho == (H - 1) / 2 + 1 and Wo == (W - 1) / 2 + 1. */
int dcf_maxpool3x3s2_fwd(int dtype, const void *x, void *y, int B, int H, int W, int Ho, int Wo, int C,
                         dcf_stream_t stream);
int dcf_maxpool3x3s2_bwd(int dtype, const void *x, const void *y, const void *gy, void *gx, int B, int H, int W,
                         int Ho, int Wo, int C, dcf_stream_t stream);
/* Same pooling with the arg-max recorded: idx uint32 [B][Ho][Wo][C/4], one byte per channel = window position dh*3+dw of
 * the first maximum in scan order; the backward is then a gather over (idx, gy) that never re-reads x. */
int dcf_maxpool3x3s2_fwd_idx(int dtype, const void *x, void *y, uint32_t *idx, int B, int H, int W, int Ho, int Wo, int C,
                             dcf_stream_t stream);
int dcf_maxpool3x3s2_bwd_idx(int dtype, const uint32_t *idx, const void *gy, void *gx, int B, int H, int W, int Ho, int Wo, int C,
                             dcf_stream_t stream);
/* Heads (model.py:168-172 softmax pairs, :116-137 box decode, :204 concat):
 * head [B,h,w,Cp] (first 18 channels = 4 class logits + 14 offsets) ->
 * pred [B,32,h,w] fp32 NCHW = cat(softmax2,softmax2, reg14, decode(reg14, anchors[14,h,w])). */
int dcf_head_fwd(int dtype, const void *head, int Cp, const float *anchors, float *pred, int B, int h, int w,
                 dcf_stream_t stream);
/* gpred [B,32,h,w] fp32 -> ghead [B,h,w,Cp] (dtype), pad channels zero. */
int dcf_head_bwd(int dtype, const void *head, int Cp, const float *anchors, const float *pred, const float *gpred,
                 void *ghead, int B, int h, int w, dcf_stream_t stream);

/* Train-mode BatchNorm2d (model.py:20,24,29 with the module in .train(): batch statistics, momentum 0.1,
 * eps 1e-5).  fwd: batch mean / invstd (fp32 [C], kept for backward), running stats updated in place
 * (unbiased variance) when non-NULL, y = act(gamma*(x-mean)*invstd + beta + res).
 * bwd: dgamma/dbeta written (not accumulated), dx = gamma*invstd*(g - dbeta/M - xhat*dgamma/M).
 * ws: dcf_bn_workspace_bytes(C). */
size_t dcf_bn_workspace_bytes(int C);
int dcf_bn_train_fwd(int dtype, const void *x, const float *gamma, const float *beta, const void *res, void *y,
                     float *mean, float *invstd, float *running_mean, float *running_var, int64_t npix, int C,
                     float eps, float momentum, int relu, void *ws, dcf_stream_t stream);
int dcf_bn_train_bwd(int dtype, const void *g, const void *x, const float *mean, const float *invstd, const float *gamma,
                     float *dgamma, float *dbeta, void *dx, int64_t npix, int C, void *ws, dcf_stream_t stream);

/* ------------------------------------------------------------------ fusion
 * SURVEY.md App. D (reference: model.py:199-203 TODO).  Per sample.
 * (1) per-point camera feature: fp [n][Cf] = bilinear(F [Hf][Wf][Cf], u/4-0.5, v/4-0.5), border clamp; all n_max rows of fp are
 *     written (zeros from *count_dev on: fp needs no clearing) */
int dcf_point_sample_fwd(int dtype, const void *fmap, int Hf, int Wf, int Cf, const float *uv, const int32_t *count_dev,
                         int n_max, void *fp, dcf_stream_t stream);
/*     backward: gF[tap] += w_tap * gfp (fp32 atomics into gfmap fp32 [Hf][Wf][Cf]) */
int dcf_point_sample_bwd(int dtype, const void *gfp, int Hf, int Wf, int Cf, const float *uv, const int32_t *count_dev,
                         int n_max, float *gfmap, dcf_stream_t stream);
/*     The B frames of a batch in one launch each (grid.y = frame): fmap / gfmap [B][Hf][Wf][Cf], uv frame b at uv + b * uv_fstride
 *     floats, count_dev [B], fp / gfp [B][n_max][Cf].  Same results as B single-frame calls. */
int dcf_point_sample_fwd_batch(int dtype, const void *fmap, int Hf, int Wf, int Cf, const float *uv, int64_t uv_fstride,
                               const int32_t *count_dev, int n_max, void *fp, int B, dcf_stream_t stream);
int dcf_point_sample_bwd_batch(int dtype, const void *gfp, int Hf, int Wf, int Cf, const float *uv, int64_t uv_fstride,
                               const int32_t *count_dev, int n_max, float *gfmap, int B, dcf_stream_t stream);
/* (2) per BEV pixel: hsum[p][c] = sum_k relu(P[idx_k][c] + W1d[c][0..2].(dx,dy,z) + b1[c]),
 *     cnt[p] = number of valid neighbours.  P [n][Cb] (dtype); w1d fp32 [Cb][3]; b1 fp32 [Cb]. */
int dcf_fusion_gather_fwd(int dtype, const void *P, const float *xyz, const int32_t *idx, int K, int h, int w,
                          int stride, float xs, float xo, float ys, float yo, const float *w1d, const float *b1,
                          int Cb, void *hsum, float *cnt, dcf_stream_t stream);
/*     batch form: P [B][p_rows][Cb], xyz frame b at xyz + b * xyz_fstride floats, idx [B][K][h][w], hsum [B][h][w][Cb], cnt [B][h*w] */
int dcf_fusion_gather_fwd_batch(int dtype, const void *P, int64_t p_rows, const float *xyz, int64_t xyz_fstride, const int32_t *idx,
                                int K, int h, int w, int stride, float xs, float xo, float ys, float yo, const float *w1d,
                                const float *b1, int Cb, void *hsum, float *cnt, int B, dcf_stream_t stream);
/*     backward: recompute the ReLU mask; gP[idx_k] += m*gh (fp32 atomics, gP fp32 [n][Cb]);
 *     gw1d[c][j] += sum m*gh*delta_j ; gb1[c] += sum m*gh. */
int dcf_fusion_gather_bwd(int dtype, const void *P, const float *xyz, const int32_t *idx, int K, int h, int w,
                          int stride, float xs, float xo, float ys, float yo, const float *w1d, const float *b1,
                          int Cb, const void *ghsum, float *gP, float *gw1d, float *gb1, dcf_stream_t stream);
/* y[p][c] += cnt[p]*b2[c]  (the fc2 bias of the K-sum), and its gradient gb2[c] += sum_p cnt[p]*gy[p][c]. */
int dcf_rowscale_bias_fwd(int dtype, void *y, const float *cnt, const float *b2, int64_t npix, int C, dcf_stream_t stream);
int dcf_rowscale_bias_bwd(int dtype, const void *gy, const float *cnt, float *gb2, int64_t npix, int C, dcf_stream_t stream);
/* (version 201) the same bias gradient and, in the same pass, the gradient that goes on into the stage's last block:
 *     gout[p][c] = y[p][c] > 0 ? gy[p][c] : 0 ;  gb2[c] += sum_p cnt[p]*gy[p][c]   (gout is its own tensor: the fusion branch still
 *     reads the unmasked gy).  Replaces dcf_rowscale_bias_bwd + the in-place dcf_relu_bwd_chansum at a fusion site. */
int dcf_relu_mask_rowscale_bwd(int dtype, const void *gy, const void *y, const float *cnt, void *gout, float *gb2, int64_t npix, int C,
                               dcf_stream_t stream);
/* dtype <-> fp32 casts of whole buffers (gradient hand-offs of the fusion path). */
int dcf_cast(int dtype_src, const void *src, int dtype_dst, void *dst, int64_t n, dcf_stream_t stream);

/* ------------------------------------------------------------------- optimiser
 * Fused Adam over the flat fp32 parameter arena (train.py:28,36: Adam(lr, betas=(beta1,0.999)),
 * eps 1e-8, no weight decay, bias-corrected like torch.optim.Adam). gscale multiplies the gradient
 * (1/world_size after the all-reduce). */
int dcf_adam_step(float *params, const float *grads, float *m, float *v, int64_t n, float lr, float beta1,
                  float beta2, float eps, int step, float gscale, dcf_stream_t stream);

/* (version 202) The guarded Adam step of train.py:28,36 (csrc/amp.hip): loss scaling -- a static scale, or the dynamic schedule
 * of torch.amp.GradScaler -- an exact skip of a step whose gradient holds a NaN or an inf, and global-norm clipping, decided on the
 * device (the host never waits).  One block of device memory holds the state (8-byte aligned; zero it, then set scale_next):
 *   scale_next      the scale the NEXT backward is seeded with (loss * scale_next); written by dcf_amp_update
 *   scale_in        the scale the current backward used: latched from scale_next by dcf_grad_stats, read by dcf_amp_update
 *   growth_tracker  clean steps since the last change of a dynamic scale (torch._amp_update_scale_)
 *   found_inf       1 = the last dcf_amp_update skipped its step
 *   applied_steps / skipped_steps   Adam's bias-correction count t = applied_steps
 *   grad_norm       L2 norm of the gradient Adam sees (sqrt(sum g^2) * |gscale_host| / scale_in)
 *   clip_coef       min(1, max_norm / (grad_norm + 1e-6)); exactly 1 when not clipped
 *   gscale, lr_over_bc1, inv_sqrt_bc2   the step's Adam scalars (gscale_host / scale_in * clip_coef, and dcf_adam_step's host
 *                   expressions for t, in double, rounded to float)
 *   part_sum / part_flag   workspace: dcf_grad_stats' per-workgroup partial sums of g^2 and non-finite flags
 * A step is three launches on one stream, after the gradient arena is final (all-reduced):
 *   dcf_grad_stats(grads, n, state)  reads the arena once (4n bytes, fixed grid of DCF_AMP_PARTS workgroups: bit-reproducible)
 *   dcf_amp_update(state, ...)       one workgroup: found_inf = any NaN / +-inf, or a non-finite norm while clipping
 *                                     (max_norm > 0; <= 0 = no clipping); dynamic != 0: GradScaler's rule (back off on found_inf,
 *                                     grow after growth_interval clean steps); static: the scale stays
 *   dcf_adam_step_guarded(...)       dcf_adam_step's arithmetic with the state's scalars; stores nothing when found_inf is set
 * Edges (tests/test_gpu_optim_edges.py): the partial sums of g^2 are fp32, so finite gradients whose squares overflow give an infinite
 * grad_norm -- while clipping that skips the step (found_inf = 1), without clipping the step is applied with clip_coef 1; a growth
 * that would overflow float leaves the scale and resets the tracker; a skipped step leaves applied_steps, gscale, lr_over_bc1 and
 * inv_sqrt_bc2 as they were; n == 0 gives grad_norm 0 and clip_coef 1.
 * grads must be 16-byte aligned. */
#define DCF_AMP_PARTS 1024
typedef struct dcf_amp_state {
    float scale_in, scale_next;
    int32_t growth_tracker, found_inf;
    int64_t applied_steps, skipped_steps;
    float grad_norm, clip_coef;
    float gscale, lr_over_bc1, inv_sqrt_bc2;
    int32_t pad_[3];
    float part_sum[DCF_AMP_PARTS];
    int32_t part_flag[DCF_AMP_PARTS];
} dcf_amp_state;
int dcf_grad_stats(const float *grads, int64_t n, dcf_amp_state *state, dcf_stream_t stream);
int dcf_amp_update(dcf_amp_state *state, float gscale_host, int dynamic, double growth_factor, double backoff_factor,
                   int growth_interval, float max_norm, float lr, float beta1, float beta2, dcf_stream_t stream);
int dcf_adam_step_guarded(float *params, const float *grads, float *m, float *v, int64_t n, float beta1, float beta2, float eps,
                          const dcf_amp_state *state, dcf_stream_t stream);

/* (version 202 still: added without a new minor) The training recipe's optimiser step (`lr_schedule` / `weight_decay` / `ema_decay`,
 * DESIGN.md section 15; csrc/optim.hip): dcf_adam_step / dcf_adam_step_guarded with torch.optim.AdamW's decoupled weight decay and
 * an exponential moving average of the parameters in the same pass.  Per element, fp32, nothing contracted, in this order:
 *     gk = g * gscale ;  m' = b1*m + (1-b1)*gk ;  v' = b2*v + (1-b2)*gk*gk                    (dcf_adam_step's expressions)
 *     q  = decays(i) ? p * decay_mul : p ;  p' = q - lr_over_bc1 * m' / (sqrtf(v') * inv_sqrt_bc2 + eps)
 *     e' = e + ema_omd * (p' - e)                                                              (ema != NULL only)
 * decay_mul = (float)(1 - lr * weight_decay) and ema_omd = (float)(1 - decay) come from the host.  state == NULL: lr_over_bc1 and
 * inv_sqrt_bc2 are dcf_adam_step's host expressions for `step`.  state != NULL: those two and gscale are read from the state (lr,
 * step and gscale are ignored), and with found_inf set NOTHING is stored -- not p, m, v and not ema.
 * decay_bits: one bit per float4 group -- group j is elements 4j .. 4j+3, its bit is bit j % 64 of word j / 64 (ceil(ceil(n/4)/64)
 * words; a tail group of fewer than four elements uses its bit like any other); NULL = every element decays.
 * With decay_mul == 1, ema == NULL the stores are bit for bit dcf_adam_step's (state == NULL) / dcf_adam_step_guarded's.
 * The products are formed left to right ((1-b2)*gk)*gk, (lr_over_bc1*m') / (...); denormals are kept, the divide and the square root
 * are IEEE's, and nothing is clamped: with eps == 0 an element with v' == 0 gets 0 / 0 = NaN (m' == 0) or -+inf, in all three kernels.
 * params, grads, m, v, ema 16-byte aligned, decay_bits 8-byte aligned; ema must not overlap the other four; ema_omd in [0, 1].
 * A learning-rate schedule needs no entry of its own: the step's rate is passed by value here, to dcf_adam_step and to dcf_amp_update. */
int dcf_adamw_ema_step(float *params, const float *grads, float *m, float *v, float *ema, const uint64_t *decay_bits, int64_t n,
                       float lr, float beta1, float beta2, float eps, int step, float gscale, float decay_mul, float ema_omd,
                       const dcf_amp_state *state, dcf_stream_t stream);

/* (version 202 still: the entry adds to the ABI without changing any of it; probe for the symbol) Parameter groups in the optimiser
 * pass (`param_groups`; csrc/optim.hip): dcf_adamw_ema_step with a second side table.  group_ids (device) holds
 * one byte per float4 group of the arena (ceil(n/4) bytes; group j = elements 4j .. 4j+3), the id g of the group's parameter group,
 * 0 .. ngroups-1; groups (HOST, ngroups <= DCF_ADAM_MAX_GROUPS entries, copied into the kernel argument) holds per id
 * {mu, decay_mul, frozen}.  Per element of a float4 group with id g, fp32, nothing contracted:
 *     frozen_g :  skipped -- g is not read and p, m, v, e are not stored: they keep their bits whatever g holds (NaN included)
 *     else     :  gk, m', v' as dcf_adamw_ema_step ;  q = decays(i) ? p * decay_mul_g : p
 *                 lr_g = lr_over_bc1 * mu_g                                  (one fp32 product; lr_over_bc1 as in dcf_adamw_ema_step)
 *                 p' = q - lr_g * m' / (sqrtf(v') * inv_sqrt_bc2 + eps) ;  e' = e + ema_omd * (p' - e)       (ema != NULL only)
 * decay_mul_g = (float)(1 - lr * mu_g * weight_decay) comes from the host.  With mu == 1, decay_mul_g == decay_mul and nothing frozen
 * the stores are dcf_adamw_ema_step's bits.  state != NULL: the guarded form, found_inf set stores nothing.  Alignment and aliasing
 * rules are dcf_adamw_ema_step's; mu must be finite and >= 0, decay_mul finite.  An id of ngroups or more (the ids live on the device:
 * the caller checks them where it builds them) makes its float4 group behave as frozen. */
#define DCF_ADAM_MAX_GROUPS 16
typedef struct { float mu, decay_mul; int32_t frozen; } dcf_adam_group;
int dcf_adamw_ema_step_groups(float *params, const float *grads, float *m, float *v, float *ema, const uint64_t *decay_bits,
                              const uint8_t *group_ids, int ngroups, const dcf_adam_group *groups, int64_t n, float lr, float beta1,
                              float beta2, float eps, int step, float gscale, float ema_omd, const dcf_amp_state *state,
                              dcf_stream_t stream);

/* (version 202 still: tests/test_amp_host.py pins the number, and the entry adds to the ABI without changing any of it; probe for the
 * symbol) Gradient accumulation (`grad_accum_steps`; csrc/optim.hip): one streaming pass over n floats,
 *     mode 0   dst[i] = src[i]
 *     mode 1   dst[i] = dst[i] + src[i]          one fp32 add per element, nothing contracted, no atomics
 * on the whole gradient arena or on a sub-range of it (a gradient bucket): dst and src need only be 4-byte aligned.  When they share
 * their offset modulo 16 bytes the pass moves one float4 per lane (a scalar head up to the first 16-byte boundary, a ragged tail
 * element by element), otherwise one float per lane; the result does not depend on which.  n == 0 launches nothing.  NULL pointers,
 * n < 0, another mode, or [dst, dst + n) overlapping [src, src + n) are errors: nothing is launched. */
int dcf_grad_accumulate(float *dst, const float *src, int64_t n, int mode, dcf_stream_t stream);

/* dcf_fusion_gather_bwd driven by dcf_fusion_invert's pairs (Cb in {64,128,192,256}): same sums, no idx -> point -> row
 * dependency chain.  The map's pairs are [*e_begin, *e_end) = start[g*(n_max+1)], start[g*(n_max+1)+n_max];
 * max_entries = K*h*w sizes the grid.
 * workspace (optional, dcf_fusion_gather_bwd_workspace_bytes(Cb), ZERO before its first use, left zero = reusable): with it the
 * workgroups' sums of gw1d / gb1 go through 16 copies of the accumulators that the last-arriving workgroup folds (16 instead of
 * 256 same-address atomics per word); NULL: float atomics straight onto gw1d / gb1.  Calls that share a workspace must be
 * ordered on one stream. */
size_t dcf_fusion_gather_bwd_workspace_bytes(int Cb);
int dcf_fusion_gather_bwd_inv(int dtype, const void *P, const float *xyz, const int32_t *e_begin, const int32_t *e_end,
                              const int32_t *ent_pix, const int32_t *ent_pt, int max_entries, int h, int w, int stride, float xs,
                              float xo, float ys, float yo, const float *w1d, const float *b1, int Cb, const void *ghsum, float *gP,
                              float *gw1d, float *gb1, void *workspace, dcf_stream_t stream);
/* The B frames of a batch (consecutive maps of one dcf_fusion_invert call) in one launch: P / gP [B][p_rows][Cb], xyz frame b at
 * xyz + b * xyz_fstride floats, frame b's e_begin / e_end at + b * seg_fstride ints (= n_max + 1 for consecutive maps), ghsum
 * [B][h][w][Cb]; gw1d / gb1 accumulate over the frames.  B <= 64. */
int dcf_fusion_gather_bwd_inv_batch(int dtype, const void *P, int64_t p_rows, const float *xyz, int64_t xyz_fstride, const int32_t *e_begin,
                                    const int32_t *e_end, int64_t seg_fstride, const int32_t *ent_pix, const int32_t *ent_pt, int max_entries,
                                    int h, int w, int stride, float xs, float xo, float ys, float yo, const float *w1d, const float *b1, int Cb,
                                    const void *ghsum, float *gP, float *gw1d, float *gb1, void *workspace, int B, dcf_stream_t stream);

/* The same sums with gP [B][p_rows][Cb] in the COMPUTE dtype and ZERO on entry (rows of points no pixel chose stay zero): a
 * point whose pairs all sit in one 16..128-pair slice of the sorted list has one writer and its row is stored whole; a point
 * whose run crosses slices is summed in an fp32 row of direct_ws by the slices of its run, and the last of them (a ticket per
 * row) stores it.  direct_ws: dcf_fusion_gather_bwd_direct_workspace_bytes(max_entries, Cb, B) bytes, zero on entry, left zero.
 * No fp32 accumulator the size of gP to fill before the launch and to cast after it.  (Reference: the autograd of
 * model.py:210-219 -- index_select / cat / Linear / ReLU / sum -- for dL/d(point features).) */
size_t dcf_fusion_gather_bwd_direct_workspace_bytes(int max_entries, int Cb, int B);
int dcf_fusion_gather_bwd_direct_batch(int dtype, const void *P, int64_t p_rows, const float *xyz, int64_t xyz_fstride,
                                       const int32_t *e_begin, const int32_t *e_end, int64_t seg_fstride, const int32_t *ent_pix,
                                       const int32_t *ent_pt, int max_entries, int h, int w, int stride, float xs, float xo, float ys,
                                       float yo, const float *w1d, const float *b1, int Cb, const void *ghsum, void *gP, float *gw1d,
                                       float *gb1, void *workspace, void *direct_ws, int B, dcf_stream_t stream);

/* The same sums with ONE writer per point row (a wave owns a range of points and all their pairs): gP [n_rows][Cb] in the compute
 * dtype, every row written (zeros where no pixel chose the point) -- no zero-filled fp32 accumulator, no float atomics on gP, no
 * cast afterwards.  start = the map's slice of dcf_fusion_invert's start array (n_rows + 1 entries are read, n_rows <= n_max). */
int dcf_fusion_gather_bwd_pts(int dtype, const void *P, const float *xyz, const int32_t *start, int n_rows, const int32_t *ent_pix,
                              const int32_t *ent_pt, int max_entries, int h, int w, int stride, float xs, float xo, float ys, float yo,
                              const float *w1d, const float *b1, int Cb, const void *ghsum, void *gP, float *gw1d, float *gb1,
                              dcf_stream_t stream);

/* ------------------------------------------------------------- deterministic mode (`deterministic: true`)
 * The fusion backward and the loss with every sum in ONE order fixed by shapes and data: no float atomics (csrc/fusion_det.hip,
 * the DET instantiations of csrc/loss.hip).  Same mathematics as the entries above, results equal to theirs to rounding.
 *
 * dcf_inv_sort_segments: segment s = keys[start[s] .. start[s+1]) (s < nseg; start has nseg + 1 entries) is sorted ascending in
 *   place; keys must be unique inside a segment.  Applied to ent_pix after dcf_fusion_invert it makes the order of a point's pairs
 *   independent of timing (ent_pt is constant inside a segment).  scratch: as many ints as keys (used by segments beyond 4096 keys).
 * dcf_cam_invert: inverse of the point sampler's bilinear scatter.  start int32 [B * (Hf*Wf + 1)], segment b * (Hf*Wf + 1) + pixel =
 *   the keys point * 4 + tap (tap 0..3 = (y0,x0) (y0,x1) (y1,x0) (y1,x1) of the sampler, border clamp included) that touch the
 *   pixel, ascending; ent / scratch int32 [B * 4 * n_max]; ws of dcf_cam_invert_workspace_bytes.  uv [B][rows][2], frames uv_fstride
 *   floats apart; points below min(count_dev[b], n_max) count.
 * dcf_point_sample_bwd_det: gfmap fp32 [B][Hf][Wf][Cf] = the scatter of gfp [B][gfp_rows][Cf] through that map, every row STORED
 *   once (zeros where no point touches: no zero-fill before).  Cf in {64, 128, 192, 256}.
 * dcf_fusion_gather_bwd_det: dcf_fusion_gather_bwd_direct_batch on SORTED maps: gP [B][p_rows][Cb] in the compute dtype, every row
 *   stored (no zero-fill), gw1d / gb1 accumulated (+=) once by a second small launch.  start = the start entries of the B
 *   consecutive maps of this site (frames n_max + 1 apart).  workspace of dcf_fusion_gather_bwd_det_workspace_bytes, contents free.
 * dcf_rowscale_bias_bwd_det: gb2[c] += sum_p cnt[p] * gy[p][c]; with y and gout also gout = gy * (y > 0) (dcf_relu_mask_rowscale_bwd).
 * dcf_loss_fwd_bwd_det / dcf_loss_sample_fwd_bwd_det: the two loss entries below; loss_rows = B floats of scratch.
 * dcf_rows_fold: dst[i] += rows[0][i] + rows[1][i] + ... in row order. */
int dcf_inv_sort_segments(const int32_t *start, int nseg, int32_t *keys, int32_t *scratch, dcf_stream_t stream);
size_t dcf_cam_invert_workspace_bytes(int Hf, int Wf, int B);
int dcf_cam_invert(const float *uv, int64_t uv_fstride, const int32_t *count_dev, int n_max, int Hf, int Wf, int B, int32_t *start,
                   int32_t *ent, int32_t *scratch, void *ws, dcf_stream_t stream);
int dcf_point_sample_bwd_det(int dtype, const void *gfp, int64_t gfp_rows, int Hf, int Wf, int Cf, const float *uv, int64_t uv_fstride,
                             const int32_t *start, const int32_t *ent, float *gfmap, int B, dcf_stream_t stream);
size_t dcf_fusion_gather_bwd_det_workspace_bytes(int max_entries, int Cb, int B);
int dcf_fusion_gather_bwd_det(int dtype, const void *P, int64_t p_rows, const float *xyz, int64_t xyz_fstride, const int32_t *start,
                              int n_max, const int32_t *ent_pix, const int32_t *ent_pt, int max_entries, int h, int w, int stride,
                              float xs, float xo, float ys, float yo, const float *w1d, const float *b1, int Cb, const void *ghsum,
                              void *gP, float *gw1d, float *gb1, void *workspace, int B, dcf_stream_t stream);
size_t dcf_rowscale_bias_bwd_det_workspace_bytes(int C);
int dcf_rowscale_bias_bwd_det(int dtype, const void *gy, const void *y, const float *cnt, void *gout, float *gb2, int64_t npix, int C,
                              void *workspace, dcf_stream_t stream);
int dcf_rows_fold(const float *rows, int nrows, int n, float *dst, dcf_stream_t stream);
int dcf_loss_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                         const int64_t *ints, const float *floats, int B, int HW, float reg_gain, int reduction, float *loss,
                         float *gcls, int64_t gcls_bstride, float *greg, int64_t greg_bstride, float *loss_rows, dcf_stream_t stream);
int dcf_loss_sample_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                                int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                                int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                                int32_t *counts_out, float *loss_rows, dcf_stream_t stream);

/* ------------------------------------------------------------- detection objective (loss.py:129-189)
 * Device half of LossTotal: 2-way cross-entropy at the sampled cells of both anchors + Smooth-L1 of the encoded box
 * offsets, and their gradients (fp32 atomics into ZEROED dense maps), in one launch; *loss (zeroed) receives the scalar.
 * cls [B][4][HW] / reg [B][14][HW] fp32 with the given batch strides (elements); anchors [2][7][HW].
 * ints (int64) = B x {off_int, npos, nneg, nrow, off_float, nbox}, then per sample: positive cells, negative cells,
 * regression cells, box index of each regression cell;  floats = per sample: weight of each regression cell, boxes [nbox][7].
 * The host-side target assignment that fills them is loss.py:74-127 (numpy RNG).  reduction: 0 last sample only
 * (reference behaviour), 1 sum, 2 mean over the batch. */
int dcf_loss_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                     const int64_t *ints, const float *floats, int B, int HW, float reg_gain, int reduction,
                     float *loss, float *gcls, int64_t gcls_bstride, float *greg, int64_t greg_bstride, dcf_stream_t stream);

/* The same objective with the target assignment ON THE DEVICE (loss.py:74-127 without the host): per sample the
 * positive windows (span x span cells around each labelled box's centre cell, fp32 arithmetic as loss.py:85-86), a uniform subset
 * of pos_cap entries when there are more (loss.py:107-110), neg_count cells drawn with replacement and rejected against the
 * selected positives (loss.py:117-126), then the terms and gradients of dcf_loss_fwd_bwd -- one launch, one workgroup per sample.
 * boxes [B][max_box][box_stride] fp32 on the device (x, y, z, l, w, h, yaw first), nbox_dev int32 [B]; xs, xo, ys, yo = grid scale /
 * offset (data_import_carla.py:35-43), reduced_scale = anchor stride.  Randomness = dcf_loss_sample_rand(seed, sample, stream, index,
 * attempt), a stateless 64-bit mix (stream 1: subset keys, the pos_cap smallest (key, entry) win; stream 2: negative item `index`,
 * cell = (rand * H*W) >> 32).  Optional outputs for inspection: pos_out int32 [B][pos_cap] (-1 padded), neg_out [B][neg_count],
 * counts_out [B][2] = {selected positives, window entries}.  max_box <= 64, max_box * span^2 <= 1024, neg_count <= 512. */
uint32_t dcf_loss_sample_rand(uint64_t seed, int sample, int stream, int index, int attempt);
int dcf_loss_sample_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                            const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                            float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                            int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                            int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                            int32_t *counts_out, dcf_stream_t stream);

/* (version 202 still: added without a new minor) Hard negative mining (`loss_sampling: hard`): dcf_loss_sample_fwd_bwd with the negatives MINED
 * instead of drawn.  Windows, the positive subset (same hash streams, same seed) and all terms are those of the entry above; the
 * negatives of a sample are the min(neg_count, candidates) cells outside EVERY window entry (also those the pos_cap cut dropped)
 * with the highest key, ties by the lower cell index, listed in that order:
 *     key(cell) = max(1, max over anchors a of ord(fl32(cls[2a+1][cell] - cls[2a][cell]))),
 *     ord(d) = bits(d) ^ 0x80000000 when the sign bit is clear, ~bits(d) otherwise        (unsigned; follows the order of the floats)
 * No randomness, no duplicates, no gradient through the selection; with no candidate the negative term is absent.  An exact radix
 * select (8-bit digits, per-workgroup histograms, integer atomics only) spread over the map, then one workgroup per sample for the
 * terms.  workspace: dcf_loss_hard_workspace_bytes(B, H, W) bytes, 4-byte aligned, contents free on entry; calls that share it must
 * be ordered on one stream.  reduction 0 with neg_out == counts_out == NULL mines the last sample only.
 * Outputs for inspection: pos_out as above, neg_out int32 [B][neg_count] (-1 in unused slots), counts_out [B][3] = {selected
 * positives, window entries, selected negatives}.  Limits as above; the _det entry sums in one fixed order (loss_rows: B floats). */
size_t dcf_loss_hard_workspace_bytes(int B, int H, int W);
int dcf_loss_hard_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                          const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                          float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                          int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                          int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                          int32_t *counts_out, void *workspace, dcf_stream_t stream);
int dcf_loss_hard_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                              const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                              float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                              int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                              int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                              int32_t *counts_out, void *workspace, float *loss_rows, dcf_stream_t stream);

/* (version 202 still: added without a new minor) Dense focal classification (`loss_sampling: focal`): no
 * sampling.  P_b = the DISTINCT cells inside at least one positive window of sample b (windows as above), N_b = max(1, |P_b|).  For
 * anchor a and cell i, y = (i in P_b): p_t = cls[2a+y][i], alpha_t = y ? alpha : 1 - alpha, q = p_t < eps ? eps : p_t (a comparison:
 * a NaN score stays NaN), FL = -alpha_t (1-q)^gamma ln q, cls_b = sum FL / N_b; the gradient is taken at q,
 *     d cls_b / d cls[2a+y][i] = (alpha_t gamma (1-q)^(gamma-1) ln q - alpha_t (1-q)^gamma / q) / N_b        (gamma == 0: -alpha_t / (q N_b)),
 * and the other channel of the pair gets 0.  Every cell of a computed sample's four gcls channels is STORED (no atomics, no need for
 * the zero fill); greg receives the regression rows of the sampled modes (every window entry for regress_type 0, else the centre
 * cell) and must be zeroed.  total_b = cls_b + reg_gain * reg_b; *loss is stored, not added to: the workgroups' partial values are
 * added in a fixed order in double and rounded once, in both entries.  reduction 0 computes the last sample only.
 * terms fp32 [B][3] = (cls_b, reg_b without the gain, |P_b|), unweighted; zero rows for samples that reduction 0 leaves out.
 * alpha in (0, 1), gamma 0 or >= 1, eps in (0, 1e-3]; max_box <= 64, max_box * span^2 <= 1024, H*W < 2^30.
 * workspace: dcf_loss_focal_workspace_bytes(B, H, W) bytes, 4-byte aligned, contents free on entry; calls that share it must be
 * ordered on one stream.  The _det entry differs in the regression gradients only: summed per cell in row order instead of atomics. */
size_t dcf_loss_focal_workspace_bytes(int B, int H, int W);
int dcf_loss_focal_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                           const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                           float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, float alpha,
                           float gamma, float eps, float reg_gain, int reduction, float *loss, float *gcls, int64_t gcls_bstride,
                           float *greg, int64_t greg_bstride, float *terms, void *workspace, dcf_stream_t stream);
int dcf_loss_focal_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                               const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                               float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, float alpha,
                               float gamma, float eps, float reg_gain, int reduction, float *loss, float *gcls, int64_t gcls_bstride,
                               float *greg, int64_t greg_bstride, float *terms, void *workspace, dcf_stream_t stream);

/* (version 202 still: added without a new minor) IoU-based anchor assignment (`loss_sampling: anchor`; assign.py
 * and loss.anchor_terms are the host statements).  Anchor index j = a*H*W + i for anchor a in {0, 1} and cell i.
 * dcf_assign_anchors_iou: I(j, k) = the bird's-eye IoU of anchor j's (x, y) rectangle clipped by label k's, in fp64 on the fp32 inputs
 *   (the geometry of dcf_eval_nms mode 2); a label row k < min(nbox, max_box) with a non-finite x, y, l, w or yaw, or l <= 0 or w <= 0, is
 *   VOID: I = 0 everywhere.  best(j) = max_k I(j, k) (0 without labels), arg(j) = the lowest k attaining it; forced(k) = the j of highest
 *   I(j, k) provided that is > 0, ties to the lowest j.  target(j) = the lowest k with forced(k) == j; else arg(j) if best(j) >= pos_iou;
 *   else -1 (negative) if best(j) < neg_iou; else -2 (ignored).  A pair whose centres are further apart than the two half-diagonals
 *   together skips the clip (its value there is exactly 0).  Anchors must have l, w > 0.
 *   target int32 [B][2][H*W], best fp64 [B][2][H*W] or NULL, counts int32 [B][4] = (N_b = positive anchors, ignored anchors, anchors
 *   positive through forcing only, void labels).  All B samples are assigned.  0 < neg_iou <= pos_iou <= 1, max_box in 1..64,
 *   box_stride >= 7, H*W < 2^30.  workspace: dcf_assign_anchors_workspace_bytes(B, H, W, max_box) bytes, 8-byte aligned, contents free on
 *   entry; calls that share it must be ordered on one stream.  Integer and fp64 work in a fixed order: no atomics.
 * dcf_loss_anchor_fwd_bwd: the terms on such targets.  Classification over every j with target != -2: y = target >= 0,
 *   p_t = cls[2a+y][i], alpha_t = y ? alpha : 1 - alpha, FL and its gradient those of dcf_loss_focal_fwd_bwd (same clamp: a NaN score stays
 *   NaN), cls_b = sum FL / max(1, N_b), N_b = counts[b][0]; the other channel of the pair, and both channels of an ignored anchor, get 0.
 *   Regression over the positive j, box k = target(j), components c = 0..6: d = reg[7a+c][i] - (the encoded offset of box k against
 *   anchor (a, i), as in the other entries), reg_b = sum SmoothL1(d) / (7 max(1, N_b)).  total_b = cls_b + reg_gain * reg_b; *loss is
 *   stored: partial values added in a fixed order in double, rounded once.  reduction 0 computes the last sample only.
 *   EVERY element of the 4 gcls and 14 greg channels of a computed sample is stored: no atomics, no zero fill needed, one entry for
 *   deterministic and plain runs.  A target outside [-2, max_box) counts as ignored.  terms fp32 [B][3] = (cls_b, reg_b without the
 *   gain, N_b), zero rows for samples that reduction 0 leaves out.  alpha, gamma, eps as for the focal entry.
 *   workspace: dcf_loss_anchor_workspace_bytes(B, H, W) bytes, 4-byte aligned, contents free on entry. */
size_t dcf_assign_anchors_workspace_bytes(int B, int H, int W, int max_box);
int dcf_assign_anchors_iou(const float *anchors, const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H,
                           int W, double pos_iou, double neg_iou, int32_t *target, double *best, int32_t *counts, void *workspace,
                           dcf_stream_t stream);
size_t dcf_loss_anchor_workspace_bytes(int B, int H, int W);
int dcf_loss_anchor_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                            const float *boxes, int max_box, int box_stride, const int32_t *target, const int32_t *counts, int B, int H,
                            int W, float alpha, float gamma, float eps, float reg_gain, int reduction, float *loss, float *gcls,
                            int64_t gcls_bstride, float *greg, int64_t greg_bstride, float *terms, void *workspace, dcf_stream_t stream);

/* (version 202 still: added without a new minor) Rotated-IoU regression term on the targets above (`iou_loss_gain`, DESIGN.md section
 * 26; loss.anchor_iou_terms and loss.iou_value_grad are the host statements).  For every positive anchor j of a computed sample (target
 * in [0, max_box)): q = label row target(j) (x, y, z, l, w, h, yaw; z at mid-height), p = the head's decode of the anchor's seven
 * offsets r without the yaw wrap, in fp64 on the fp32 inputs: x = r0 diag + a0, y = r1 diag + a1, z = r2 a5 + a2, l = exp(r3) a3,
 * w = exp(r4) a4, h = exp(r5) a5, yaw = r6 + a6, diag = sqrt(a3^2 + a4^2).  IoU = the 3-D IoU of dcf_eval_nms mode 2's geometry (kind 0)
 * or its bird's-eye IoU (kind 1), computed by clipping the edges of each rectangle in the other, relative to q's centre.
 *   L_b = sum_j (1 - IoU_j) / max(1, N_b), N_b = counts[b][0];   *loss += sum over the computed samples of wsample iou_gain L_b
 *   (the workgroups' partial sums folded in a fixed order in double; *loss is read, so it must hold the value of dcf_loss_anchor_fwd_bwd,
 *   launched before on the same stream);   greg[b][7a + c][i] += wsample iou_gain d L_b / d r_c for the positive anchors only -- one
 *   lane owns a positive's seven elements, every other element of greg keeps its bits.  A disjoint pair adds 1 / max(1, N_b) to L_b and
 *   seven zeros; a pair with a non-finite p or q gives NaN (value and its own seven gradients).  No atomics: one entry for deterministic
 *   and plain runs.  iou_terms fp32 [B][2] = (sum_j IoU_j / max(1, N_b), N_b), zero rows for the samples reduction 0 leaves out.
 *   iou_map fp64 [B][2][H*W] or NULL: IoU_j for a positive anchor, 0 for every other anchor of a computed sample.
 *   workspace: dcf_loss_anchor_iou_workspace_bytes(B, H, W) bytes, 8-byte aligned, contents free on entry. */
size_t dcf_loss_anchor_iou_workspace_bytes(int B, int H, int W);
int dcf_loss_anchor_iou_fwd_bwd(const float *reg, int64_t reg_bstride, const float *anchors, const float *boxes, int max_box,
                                int box_stride, const int32_t *target, const int32_t *counts, int B, int H, int W, int kind,
                                float iou_gain, int reduction, float *loss, float *greg, int64_t greg_bstride, float *iou_terms,
                                double *iou_map, void *workspace, dcf_stream_t stream);

/* ------------------------------------------------- evaluation post-processing
 * What /root/reference/test.py:88-206 does on the host, box by box.
 * dcf_eval_score_filter: test.py:88-108.  pred [B][32][h][w] fp32 (the model output: scores in channels 2a+1, decoded boxes in
 *   18+7a..18+7a+6 for anchor a); boxes_out [B][cap][7] receives, per sample, anchor 0's boxes with score > threshold in raster
 *   order, then anchor 1's; count_out[b] = how many passed (may exceed cap: rows past cap are dropped).
 * dcf_eval_nms: test.py:110-175.  Greedy suppression in INPUT order: keep[i] = 1 iff box i overlaps no earlier kept box.
 *   mode 0 = separating-axis test of the bird's-eye rectangles (NMS_SAT; touching counts), mode 1 = 3-D IoU > iou_threshold with the
 *   kept box's centre nudged by 1e-4 (NMS_IOU), mode 2 = see the ranked evaluation below.  boxes [n_max][7] fp32 (x, y, z, l, w, h, yaw); count_dev (may be NULL) = number of
 *   valid rows on the device; n_max <= 4096.  ws: dcf_eval_nms_workspace_bytes(n_max).
 * dcf_eval_match: test.py:177-206.  tp_counters[t] += number of predictions whose bird's-eye IoU with any labelled box
 *   (ref row [9], last column == 1) exceeds thresholds_dev[t] (fp64, on the device). */
int dcf_eval_score_filter(const float *pred, int B, int h, int w, float threshold, int cap, float *boxes_out, int32_t *count_out,
                          dcf_stream_t stream);
size_t dcf_eval_nms_workspace_bytes(int n_max);
int dcf_eval_nms(const float *boxes, const int32_t *count_dev, int n_max, int mode, double iou_threshold, int32_t *keep, int32_t *nkeep,
                 void *ws, dcf_stream_t stream);
int dcf_eval_match(const float *pred_boxes, int npred, const float *ref_boxes, int nref_rows, const double *thresholds_dev, int nthr,
                   int32_t *tp_counters, dcf_stream_t stream);

/* (version 202 still: added without a new minor) Ranked evaluation (`eval_metric: ranked`): score-ordered
 * suppression, one-to-one matching and KITTI R40 average precision, decided on integer keys and fp64 geometry; evalrank.py is the
 * host statement.  A candidate is (anchor a, pixel px) of a sample, index a*h*w + px; its key is
 * (orderable_u32(score) << 32) | (0xFFFFFFFF - index), larger first (score descending, ties to the lower index).
 * dcf_eval_rank_filter: the candidates with score > threshold in rank order: boxes_out [B][cap][7], scores_out [B][cap];
 *   total_out[b] = how many passed, count_out[b] = min(total, cap); with total > cap exactly the cap highest-ranked are written.  Rows
 *   >= count are left untouched.  ws: dcf_eval_rank_workspace_bytes(B, h, w).
 * dcf_eval_nms mode 2: bird's-eye IoU of the (x, y) rectangles > iou_threshold (no nudge; a zero-area box gives NaN = no overlap).
 * dcf_eval_match_ranked: per threshold t (bit t of tpmask[i], at most 16), the survivors (keep[i] != 0, i < *count_dev) in row order
 *   each take the labelled row (ref row [9], last column == 1) of highest bird's-eye IoU among the rows not yet taken at t (ties: the
 *   lower row); the pair counts iff that IoU > thresholds_dev[t], and only then is the row taken.  tpmask [n_max] receives rows
 *   < *count_dev.  n_max <= 4096, R <= 4096.  ws: dcf_eval_match_ranked_workspace_bytes(n_max, R).
 * dcf_eval_accumulate: appends (score, tpmask) of one sample's survivors, in order, at state[0] of acc_scores / acc_tpmask
 *   [capacity]; state (int64 [4], on the device) = {cursor, labelled rows seen, samples with total > n_max, unused}.  The cursor keeps
 *   counting past capacity; nothing is written past it.
 * dcf_eval_ap: the min(cursor, capacity) detections ordered by (score descending, accumulation index ascending); per threshold t
 *   out_counts[t] = c_N and out_ap[t] = (P_1 + ... + P_40) / 40 with P_j = max{ c_k / k : 40 c_k >= j n_gt } (0 for the empty set;
 *   NaN when n_gt == 0).  ws: dcf_eval_ap_workspace_bytes(capacity). */
size_t dcf_eval_rank_workspace_bytes(int B, int h, int w);
int dcf_eval_rank_filter(const float *pred, int B, int h, int w, float threshold, int cap, float *boxes_out, float *scores_out,
                         int32_t *count_out, int32_t *total_out, void *ws, dcf_stream_t stream);
size_t dcf_eval_match_ranked_workspace_bytes(int n_max, int R);
int dcf_eval_match_ranked(const float *boxes, const int32_t *keep, const int32_t *count_dev, int n_max, const float *ref_boxes, int R,
                          const double *thresholds_dev, int nthr, uint32_t *tpmask, void *ws, dcf_stream_t stream);
int dcf_eval_accumulate(const float *scores, const uint32_t *tpmask, const int32_t *keep, const int32_t *count_dev, const int32_t *total_dev,
                        int n_max, const float *ref_boxes, int R, float *acc_scores, uint32_t *acc_tpmask, int64_t capacity, int64_t *state,
                        dcf_stream_t stream);
size_t dcf_eval_ap_workspace_bytes(int64_t capacity);
int dcf_eval_ap(const float *acc_scores, const uint32_t *acc_tpmask, const int64_t *state, int64_t capacity, int nthr, double *out_ap,
                int64_t *out_counts, void *ws, dcf_stream_t stream);

/* (version 202 still: added without a new minor) KITTI-style protocol on the ranked evaluation (`eval_protocol: kitti`, DESIGN.md
 * section 22; evalkitti.py is the host statement): difficulty levels, a third outcome (ignored) and the 3-D IoU.  Difficulty d is
 * 0 easy, 1 moderate, 2 hard; a label row (ref row [9], last column == 1) has a level 0..3 (levels == NULL: all 0) and is COUNTED at
 * d iff level <= d, else IGNORED.  Mask words carry bit 10 d + t for threshold t (at most 10), one word per metric m (0 bird's-eye,
 * 1 3-D): arrays [2][n_max] or [2][capacity].  The entries above are not affected.
 * dcf_eval_det_flags: per candidate i < *count_dev the eight corners (the bird's-eye rectangle at z - h/2 and z + h/2) through
 *   crt_host ([4][3] fp32 ON THE HOST, read at the call: [x, y, z, 1] . C = (u d, v d, d)) in fp64, d = ((x C02 + y C12) + z C22) + C32
 *   and likewise u d, v d; corners with d > 0 only, u clamped to [0, image_w], v to [0, image_h]; height and area of the enclosing 2-D
 *   box (0 with no corner in front).  flags[i] bit d iff height < min_height_host[d] (three fp64 ON THE HOST); bit 3 iff area > 0 and
 *   for one of the D rectangles of dontcare ([D][4] fp32 on the device: l, t, r, b) iw > 0, ih > 0 and iw ih / area > overlap.
 * dcf_eval_iou_levels: iou_bev, iou_3d [n_max][R] fp64 for the survivors (keep[i] != 0, i < *count_dev) against the labelled rows,
 *   NaN elsewhere; one clip gives both: ia / (a1 + a2 - ia) as dcf_eval_match_ranked, and with zov = the overlap of the z extents
 *   [z - h/2, z + h/2], iv = ia zov: iv / (a1 h1 + a2 h2 - iv).
 * dcf_eval_match_levels: per (m, d, t) independently the survivors in row order: (A) the counted row of highest IoU among those not
 *   yet taken (ties: the lower row), a true positive iff that IoU > thresholds_dev[t] and only then is the row taken; else (B) ignored
 *   iff an ignored row has IoU > t (never taken); else (C) ignored iff flags[i] has bit d or bit 3.  tpmask / igmask [2][n_max] are
 *   zeroed and receive the bits.  n_max <= 4096, R <= 4096.
 * dcf_eval_accumulate_levels: appends (score, tpmask[2], igmask[2]) of the survivors at state[0] of acc_scores [capacity],
 *   acc_tpmask / acc_igmask [2][capacity]; state (int64 [8], on the device) = {cursor, counted rows seen at d = 0, 1, 2, samples with
 *   total > n_max, unused x 3}.  The cursor keeps counting past capacity; nothing is written past it.
 * dcf_eval_ap_levels: dcf_eval_ap per (m, d, t), at index (3 m + d) nthr + t, over the detections NOT ignored there (k counts those
 *   that stay) and n_gt = state[1 + d]: out_ap, out_tp = true positives, out_ignored = detections ignored.
 *   ws: dcf_eval_ap_levels_workspace_bytes(capacity). */
int dcf_eval_det_flags(const float *boxes, const int32_t *count_dev, int n_max, const float *crt_host, const float *dontcare, int D, int image_h,
                       int image_w, const double *min_height_host, double overlap, uint32_t *flags, dcf_stream_t stream);
int dcf_eval_iou_levels(const float *boxes, const int32_t *keep, const int32_t *count_dev, int n_max, const float *ref_boxes, int R, double *iou_bev,
                        double *iou_3d, dcf_stream_t stream);
int dcf_eval_match_levels(const double *iou_bev, const double *iou_3d, const int32_t *keep, const int32_t *count_dev, int n_max, const float *ref_boxes,
                          const int32_t *levels, int R, const uint32_t *flags, const double *thresholds_dev, int nthr, uint32_t *tpmask,
                          uint32_t *igmask, dcf_stream_t stream);
int dcf_eval_accumulate_levels(const float *scores, const uint32_t *tpmask, const uint32_t *igmask, const int32_t *keep, const int32_t *count_dev,
                               const int32_t *total_dev, int n_max, const float *ref_boxes, const int32_t *levels, int R, float *acc_scores,
                               uint32_t *acc_tpmask, uint32_t *acc_igmask, int64_t capacity, int64_t *state, dcf_stream_t stream);
size_t dcf_eval_ap_levels_workspace_bytes(int64_t capacity);
int dcf_eval_ap_levels(const float *acc_scores, const uint32_t *acc_tpmask, const uint32_t *acc_igmask, const int64_t *state, int64_t capacity, int nthr,
                       double *out_ap, int64_t *out_tp, int64_t *out_ignored, void *ws, dcf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DCF_HIP_H */
