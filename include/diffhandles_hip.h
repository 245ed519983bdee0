/*
 * diffhandles_hip.h -- C ABI of the MI355X (gfx950) native library behind the
 * DiffusionHandles guided-denoising edit path.
 *
 * The reference (adobe-research/DiffusionHandles) has no FFI of its own: its boundary is
 * the Python class API (diffhandles/diffusion_handles.py:15-166,
 * guided_stable_diffuser.py:22-610, stable_null_inverter.py:12-181).  These entry points
 * are what a ctypes binding of that path calls; each one cites the reference code whose
 * arithmetic it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream);
 *   - return value 0 = ok, negative = error (dh_last_error() gives the text);
 *   - no hidden device allocation on the hot path: callers pass workspaces whose size the
 *     *_workspace_bytes() queries return.  Engine handles own their weights/workspaces.
 *   - 16-bit activations are passed as raw uint16 storage; `dtype` says how to read them.
 */
#ifndef DIFFHANDLES_HIP_H
#define DIFFHANDLES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_OK 0
#define DH_ERR_ARG -1
#define DH_ERR_HIP -2
#define DH_ERR_STATE -3

#define DH_DTYPE_F16 0
#define DH_DTYPE_BF16 1
#define DH_DTYPE_F32 2

const char* dh_last_error(void);
int dh_version(void);
/* number of visible HIP devices (<=0: no GPU) */
int dh_device_count(void);

/* --------------------------------------------------------------------------------------
 * Depth re-projection: unproject -> SE(3) about the masked centroid -> project ->
 * z-buffer -> mask clean-up -> correspondence filter -> harmonic in-fill -> disparity.
 * Replaces transform_depth_pc / depth_to_world_coords / transform_point_cloud /
 * points_to_depth / poisson_solve / normalize_depth
 * (depth_transform.py:198-363, 589-641, 461-533, 643-747, 535-587, 15-28) and the cv2
 * morphology at :308-321, for a batch of n_edits rigid transforms of ONE image.
 *
 * xforms_host: n_edits x 8 doubles {ax, ay, az (unit axis, float32 values widened),
 *              cos(theta), sin(theta), tx, ty, tz} prepared on the host with NumPy so the
 *              transcendental values match the reference's.
 * grid_x/grid_y: the float32 pixel-centre coordinates torch.linspace gives (device).
 * Outputs per edit e (all device):
 *   zmap[e][res*res]       f32  z-buffered depth (inf where empty)
 *   raw_mask[e][res*res]   u8   pixel won by a foreground point
 *   clean_mask[e][res*res] u8   after CLOSE(ellipse res/50) + OPEN(ellipse res/250)
 *   disparity[e][res*res]  f32  255*(1/z - min)/(max - min), harmonically in-filled
 *   vis[e][n_fg]           u8   foreground point j is the (z, index) winner of its pixel
 *   target_xy[e][n_fg][2]  i32  projected pixel (x, y) of every foreground point
 *   corr[e][n_fg][4]       i64  (ox, oy, tx, ty), first counts[e] rows valid, in
 *                               row-major order of the original pixel
 *   counts[e][4]           i32  {n_corr, n_visible, n_inpaint, cg_iterations}
 * bounds: optional [2] f32 {lo, hi} normalisation bounds (use_input_depth_normalization),
 *         NULL = per-edit min/max of the rendered disparity.
 * ------------------------------------------------------------------------------------ */
int dh_reproject_workspace_bytes(int res, int n_fg, int n_edits, size_t* bytes);
int dh_fg_pixel_list(const uint8_t* fg_mask, int res, int32_t* fg_pix, int32_t* n_fg_dev,
                     void* workspace, size_t workspace_bytes, void* stream);
int dh_reproject_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                       int res, const float* grid_x, const float* grid_y, float inv_fx, float inv_fy,
                       double fx, double fy, int n_edits, const double* xforms_host,
                       const float* bounds,
                       float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                       uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Several rigid bodies per edit (not in the reference): dh_reproject_edits with n_objects (1..8) foreground objects.
 *   fg_pix      the objects' pixel lists, concatenated: object m owns fg_pix[obj_start[m] .. obj_start[m+1]), row-major
 *               within the object (dh_fg_pixel_list per mask, written into consecutive slices); the masks are disjoint
 *   obj_start   HOST, n_objects + 1 ints: 0 = obj_start[0] < obj_start[1] < ... < obj_start[n_objects] = n_fg
 *   xforms_host n_edits x n_objects rows of 8 doubles, edit-major: row e * n_objects + m moves object m in edit e,
 *               about the centroid of ITS OWN points (sequential float32 mean over its slice)
 * The point list is background, object 0, object 1, ...; ONE z-buffer over it (winner = min (z, point index)), so objects
 * occlude the background and each other and equal depths go to the earlier object.  vis / target_xy / corr are indexed
 * and ordered by position in fg_pix; everything else as dh_reproject_edits, which is the n_objects = 1 call of this one. */
int dh_reproject_objects_workspace_bytes(int res, int n_fg, int n_edits, int n_objects, size_t* bytes);
int dh_reproject_object_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                              int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                              const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                              int n_edits, const double* xforms_host, const float* bounds,
                              float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                              uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream);
/* Similarity transforms per object (not in the reference): dh_reproject_object_edits with a scale per camera axis and an
 * optional pivot.  Everything is as there except the transform row, which EXTENDS its 8 doubles to DH_SIMILARITY_ROW = 16:
 *   [0..7]   ax, ay, az, cos, sin, tx, ty, tz     the row of dh_reproject_edits / dh_reproject_object_edits, unchanged
 *   [8..10]  sx, sy, sz    scale along the camera axes of dh_unproject, float32 values widened; positive and finite
 *   [11..13] px, py, pz    pivot, a point in the coordinates dh_unproject returns, float32 values widened; finite
 *   [14]     has_pivot     1.0 = the object turns and scales about the pivot, 0.0 = about the centroid of its own points
 *   [15]     reserved, 0
 * With c = pivot or centroid (f32), P the unprojected point (f32), s the scale (f32):
 *   q = fl32(P - c),  q' = fl32(q * s) per component,  then the rotation of dh_reproject_edits on q' (f32 cross and dot
 *   products, the dot as (q'0 a0 + q'1 a1) + q'2 a2; f64 combination with cos / sin / 1 - cos),  (r + (double)c) + t.
 * The scale acts BEFORE the rotation: a non-uniform scale of a turned object stretches along the un-turned camera axes.
 * Scale 1 without a pivot is dh_reproject_object_edits in every output bit; a pivot equal to the centroid's own float32
 * values likewise.  Rows of different edits may give one object different pivots.  A row with a scale that is not positive
 * and finite, a pivot that is not finite, or a flag other than 0 / 1 is refused (DH_ERR_ARG) before any launch, the
 * outputs untouched.  dh_reproject_edits and dh_reproject_object_edits are the scale-1 / no-pivot calls of this entry;
 * the workspace is dh_reproject_objects_workspace_bytes' for all three. */
#define DH_SIMILARITY_ROW 16
int dh_reproject_similarity_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                                  int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                                  const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                                  int n_edits, const double* xforms_host, const float* bounds,
                                  float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                                  uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* Footprint splatting (not in the reference): dh_reproject_similarity_edits with, when footprints = 1, the triangles between
 * neighbouring foreground points of ONE object bidding in the z-buffer of the points, so an enlarged or approaching object
 * leaves no gaps between its points ("Footprint splatting", states the rules; all of it f64 in the written order).
 *   footprints     0 = dh_reproject_similarity_edits in every output byte; 1 = on
 *   max_ratio      0 = none; else finite and > 1: a triangle whose three SOURCE depths (f32) have zmax > fl32(zmin * max_ratio)
 *                  is dropped (quads across a depth step inside one mask make no sheets).  Non-zero without footprints is refused.
 *   corr_capacity  rows per edit of corr (its row stride): >= n_fg without footprints, >= res * res with; smaller is refused
 * With footprints = 1: zmap, raw_mask, clean_mask, disparity and counts as before; vis[e][j] = point j owns at least one
 * pixel; target_xy[e][j] stays the point's own rounded pixel; corr[e] has one row per foreground-owned target pixel inside the
 * cleaned mask, (ox, oy) of the owning point and (tx, ty) of the pixel, in ROW-MAJOR TARGET order (there may be more rows than
 * n_fg); counts[e][1] = number of visible points.  A refused argument is DH_ERR_ARG before any launch, the outputs untouched.
 * The workspace is dh_reproject_footprints_workspace_bytes' (with footprints = 0: dh_reproject_objects_workspace_bytes'). */
int dh_reproject_footprints_workspace_bytes(int res, int n_fg, int n_edits, int n_objects, int footprints, size_t* bytes);
int dh_reproject_footprint_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                                 int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                                 const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                                 int n_edits, const double* xforms_host, const float* bounds,
                                 float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                                 uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                                 void* workspace, size_t workspace_bytes, void* stream,
                                 int footprints, float max_ratio, int corr_capacity);
/* Copies of an object (not in the reference; DESIGN.md, "Object copies"): dh_reproject_footprint_edits with n_instances
 * INSTANCES per edit in place of one body per mask.  Instance n draws the points of mask inst_obj[n] (host array, values in
 * 0 .. n_objects - 1, every mask named at least once, n_objects <= n_instances <= 8) with row e * n_instances + n of xforms_host,
 * about the centroid of THAT MASK's points (computed once per mask) or the row's pivot.
 *   point list     background, instance 0's points (row-major), instance 1's, ...: n_pts = sum over n of |mask inst_obj[n]|
 *                  foreground points, which may exceed n_fg; ONE z-buffer, winner = min (z, point index): equal depths go to the
 *                  earlier instance, so two instances with one mask and one transform give the one-instance outputs
 *   vis, target_xy n_pts entries per edit, by point-list position
 *   corr           point-list order without footprints (a source pixel once per visible, kept instance), capacity >= n_pts;
 *                  with footprints as there (triangles between neighbouring points of ONE INSTANCE, bidder index = res * res +
 *                  point-list position), capacity >= res * res
 *   corr_inst      uint8, corr_capacity per edit, may be null: the instance n of every corr row
 * Refused (DH_ERR_ARG before any launch, outputs untouched): n_instances outside 1 .. 8, an inst_obj entry outside
 * 0 .. n_objects - 1, a mask without an instance, res * res + n_pts beyond INT_MAX, and what dh_reproject_footprint_edits refuses
 * (the row checks on all n_edits * n_instances rows).  The workspace is dh_reproject_instances_workspace_bytes' (n_pts as above).
 * dh_reproject_footprint_edits is the identity-table call of this entry (inst_obj[n] = n, corr_inst null) on its own workspace. */
int dh_reproject_instances_workspace_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances, int footprints,
                                           size_t* bytes);
int dh_reproject_instance_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                                int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                                const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                                int n_edits, const double* xforms_host, const float* bounds,
                                float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                                uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                                void* workspace, size_t workspace_bytes, void* stream,
                                int footprints, float max_ratio, int corr_capacity,
                                int n_instances, const int32_t* inst_obj, uint8_t* corr_inst);
/* Object insertion (not in the reference; DESIGN.md, "Object insertion"): dh_reproject_instance_edits with masks of a second
 * image.  Masks n_host_objects .. n_objects - 1 of fg_pix / obj_start are masks of the DONOR image (same resolution, same
 * intrinsics): their points are the unprojection of donor_depth [res][res] f32 at their pixels, their centroid the sequential
 * f32 centroid of those points.  Everything from the transform row on is shared: one z-buffer over the background and all
 * instances, masks, visibility, in-fill, normalisation.  A correspondence row of a donor instance carries its source pixel in
 * the donor image; corr_inst (required with a donor) tells which rows those are: inst_obj[corr_inst[r]] >= n_host_objects.
 * Donor pixels may coincide with host pixels.  n_host_objects = 0 is the pure insertion.
 * Refused (DH_ERR_ARG before any launch, outputs untouched), beyond what dh_reproject_instance_edits refuses: n_host_objects
 * outside 0 .. n_objects; with n_host_objects < n_objects a null donor_depth, footprints != 0 (the pixel -> list-position
 * inverse of the triangles is ambiguous when two images share pixel indices) or a null corr_inst.
 * dh_reproject_instance_edits is this entry's donor_depth = NULL, n_host_objects = n_objects call; the workspace is
 * dh_reproject_instances_workspace_bytes' under a name of its own. */
int dh_reproject_donor_workspace_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances, int footprints,
                                       size_t* bytes);
int dh_reproject_donor_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                             int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                             const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                             int n_edits, const double* xforms_host, const float* bounds,
                             float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                             uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                             void* workspace, size_t workspace_bytes, void* stream,
                             int footprints, float max_ratio, int corr_capacity,
                             int n_instances, const int32_t* inst_obj, uint8_t* corr_inst,
                             const float* donor_depth, int n_host_objects);
/* Camera moves (not in the reference; DESIGN.md, "Camera moves"): dh_reproject_donor_edits in which an edit may also move the
 * VIEWPOINT.  views [n_edits][DH_SIMILARITY_ROW] f64 and has_view [n_edits] u8 are HOST arrays: row e is the inverse motion of
 * edit e's camera as a similarity row (unit axis, cos and sin of MINUS the camera's angle, translation, scale 1, pivot, has-pivot
 * flag 1, 0); rows with has_view[e] = 0 are not read.  In an edit with a view EVERY point of the list -- the f32 background
 * point, or an instance's transformed (X, Y, Z) rounded to f32 -- goes through the view row with the arithmetic of a transform
 * row: q = fl32(P - c), f32 cross products and dot, the f64 combination, (r + (double)c) + t.  Such an edit has no clamp: a point
 * whose rint(u) or rint(v) (half to even, before any clamp) leaves 0 .. res - 1, or whose Z is not > 0, bids for no pixel and
 * yields no row; its vis is 0 and its target_xy (-1, -1).  A pixel no point reached joins the in-fill set and stays out of the
 * disparity's min / max.  The z-buffer's tie rule is unchanged (z, list index).
 *   bg_valid [res][res] u8 (device): 0 where bg_depth is in-painted (under the host's foreground and removed masks)
 *   bg_corr  [n_edits][res * res][4] i64, bg_counts [n_edits] i32 (device): the BACKGROUND rows of the view edits --
 *            background point i (source pixel i) yields (ox, oy, tx, ty) when bg_valid[i] != 0, the point owns its target
 *            pixel and that pixel lies outside the cleaned mask; ascending source pixel.  An edit without a view has none
 *            (bg_counts[e] = 0).  The layout of corr, corr_inst and counts does not change.
 * An edit without a view is computed as dh_reproject_donor_edits computes it, byte for byte; with has_view all zero (or views
 * NULL) the call IS that entry's: the three background arguments are neither read nor written and the workspace may be
 * dh_reproject_donor_workspace_bytes'.  dh_reproject_donor_edits is this entry's call without a view.
 * Refused (DH_ERR_ARG before any launch, outputs untouched), beyond what the donor entry refuses: a view with footprints != 0;
 * a view with a null bg_valid, bg_corr or bg_counts; a malformed view row (a member that is not finite, a scale that is not
 * positive, a has-pivot flag other than 0 or 1). */
int dh_reproject_camera_workspace_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances, int footprints,
                                        size_t* bytes);
int dh_reproject_camera_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                              int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                              const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                              int n_edits, const double* xforms_host, const float* bounds,
                              float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                              uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream,
                              int footprints, float max_ratio, int corr_capacity,
                              int n_instances, const int32_t* inst_obj, uint8_t* corr_inst,
                              const float* donor_depth, int n_host_objects,
                              const double* views, const uint8_t* has_view, const uint8_t* bg_valid,
                              int64_t* bg_corr, int32_t* bg_counts);
/* Object removal, the pure case (not in the reference; DESIGN.md, "Object removal"): the re-projection of the background
 * alone, for an edit that deletes its objects and moves none.  The point list is the res * res pixels of bg_depth; it runs the
 * kernels of the entries above on that part of the list: z-buffer (winner = min (z, point index)), zmap (+inf where no point
 * landed), disparity 1 / z normalised with bounds (device f32[2]) or, bounds NULL, with its own min and max, and the harmonic
 * in-fill of the pixels NO point owns (nothing is foreground: the raw and the cleaned mask are zero and are not written).
 *   zmap, disparity [res][res] f32;  counts [4] i32: {0, 0, pixels in-filled, CG iterations (negative: the in-fill failed,
 *   as in the entries above)}
 * It is NOT the empty-mask result (the normalised INPUT disparity), which the host computes without this library.
 * DH_ERR_ARG before any launch, outputs untouched: a null pointer, res outside 2 .. 32768, a workspace smaller than
 * dh_reproject_background_workspace_bytes'. */
int dh_reproject_background_workspace_bytes(int res, size_t* bytes);
int dh_reproject_background(const float* bg_depth, int res, const float* grid_x, const float* grid_y,
                            float inv_fx, float inv_fy, double fx, double fy, const float* bounds,
                            float* zmap, float* disparity, int32_t* counts,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Camera moves, the pure case: dh_reproject_background with one view row (view [DH_SIMILARITY_ROW] f64, host; NULL = no view,
 * which is dh_reproject_background launch for launch -- that entry is this one's NULL call).  With a view the background points
 * go through it as in dh_reproject_camera_edits (no clamp, out-of-frame points bid for nothing), the pixels no point reached
 * are in-filled and stay out of the min / max, and every background point with bg_valid != 0 that owns its target pixel yields
 * a row: bg_corr [res * res][4] i64, bg_counts [1] i32.  Same workspace.  DH_ERR_ARG before any launch, outputs untouched: a
 * view with a null bg_valid, bg_corr or bg_counts, a malformed view row. */
int dh_reproject_camera_background(const float* bg_depth, int res, const float* grid_x, const float* grid_y,
                                   float inv_fx, float inv_fy, double fx, double fy, const float* bounds,
                                   float* zmap, float* disparity, int32_t* counts,
                                   void* workspace, size_t workspace_bytes, void* stream,
                                   const double* view, const uint8_t* bg_valid, int64_t* bg_corr, int32_t* bg_counts);
/* The image border of the in-fill (not in the reference; DESIGN.md, "In-fill border").  infill_border: 0 = zero -- a neighbour
 * beyond the frame counts as a known 0, the diagonal of every unknown is 4: what every entry above computes -- or 1 = reflect
 * -- the mirror ghost cell x_ghost = x_self (zero normal derivative at the frame): the diagonal of an unknown is the number of
 * its 4-neighbours inside the image (4, 3 on an edge, 2 in a corner); off-diagonals and right-hand side do not change.  A hole
 * that does not touch the frame is the same system under both.  The border holds for the call, not per edit.
 *   dh_reproject_border_edits       dh_reproject_camera_edits plus infill_border; that entry is this one's infill_border = 0 call
 *   dh_reproject_border_background  dh_reproject_camera_background plus infill_border; likewise
 * The workspaces do NOT grow: size them with dh_reproject_camera_workspace_bytes (or, without a view, the donor / instance
 * query) and dh_reproject_background_workspace_bytes.  Every integer output is what it is under infill_border = 0; only the
 * disparity inside in-fill components that touch the frame, and counts[.][3], differ.
 * DH_ERR_ARG before any launch, outputs untouched, beyond what those entries refuse: infill_border other than 0 or 1. */
int dh_reproject_border_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                              int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                              const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                              int n_edits, const double* xforms_host, const float* bounds,
                              float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                              uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream,
                              int footprints, float max_ratio, int corr_capacity,
                              int n_instances, const int32_t* inst_obj, uint8_t* corr_inst,
                              const float* donor_depth, int n_host_objects,
                              const double* views, const uint8_t* has_view, const uint8_t* bg_valid,
                              int64_t* bg_corr, int32_t* bg_counts, int infill_border);
int dh_reproject_border_background(const float* bg_depth, int res, const float* grid_x, const float* grid_y,
                                   float inv_fx, float inv_fy, double fx, double fy, const float* bounds,
                                   float* zmap, float* disparity, int32_t* counts,
                                   void* workspace, size_t workspace_bytes, void* stream,
                                   const double* view, const uint8_t* bg_valid, int64_t* bg_corr, int32_t* bg_counts,
                                   int infill_border);
/* View surfaces (not in the reference; DESIGN.md, "View surfaces").  view_surfaces: 0 = every point of the list is one pixel,
 * what every entry above computes -- or 1 = in an edit WITH a view the scene is splatted as triangles: between neighbouring
 * points of one instance (the footprint rules, vertices after the view) and over every source quad of the background (vertices
 * the background points, the depth-ratio guard on the f32 bg_depth, bidder index = the source pixel of the vertex with the
 * largest weight).  All bids meet in the one z-buffer: winner = min (z, index).  Such an edit takes its rows per TARGET pixel,
 * row-major: instance rows (corr, corr_inst) for the instance-owned pixels inside the cleaned mask, background rows (bg_corr,
 * bg_counts) (o % res, o / res, tx, ty) for the pixels whose owner o < res * res has bg_valid[o] and that lie outside it; vis[j]
 * = point j owns at least one pixel; target_xy[j] stays the point's own pixel.  An edit without a view is the point path, byte
 * for byte; a call in which no edit has a view is the border entry's call, launch for launch.
 * surface_max_ratio: 0 = none, else the depth-ratio guard of the triangles (finite, > 1).  The setting holds for the call.
 *   dh_reproject_surface_edits       dh_reproject_border_edits plus the two; that entry is this one's (0, 0.f) call
 *   dh_reproject_surface_background  dh_reproject_border_background plus the two; likewise
 * Workspaces: the two queries below; with view_surfaces = 0 they equal dh_reproject_camera_workspace_bytes (footprints = 0) and
 * dh_reproject_background_workspace_bytes.  With 1 they add 24 bytes per point and edit (the stored vertices), the inverse pixel
 * map and 2 n_pts + 2 (res - 1)^2 list slots per edit.
 * DH_ERR_ARG before any launch, outputs untouched, beyond what those entries refuse: view_surfaces other than 0 or 1; a ratio
 * that is not 0 or finite and > 1; a ratio without the setting; view_surfaces = 1 with footprints = 1; view_surfaces = 1 with a
 * donor mask (n_host_objects < n_objects); corr_capacity < res * res when an edit has a view and the setting is on. */
int dh_reproject_surface_ws_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances,
                                         int view_surfaces, size_t* bytes);
int dh_reproject_surface_background_ws_bytes(int res, int view_surfaces, size_t* bytes);
int dh_reproject_surface_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                               int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                               const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                               int n_edits, const double* xforms_host, const float* bounds,
                               float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                               uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                               void* workspace, size_t workspace_bytes, void* stream,
                               int footprints, float max_ratio, int corr_capacity,
                               int n_instances, const int32_t* inst_obj, uint8_t* corr_inst,
                               const float* donor_depth, int n_host_objects,
                               const double* views, const uint8_t* has_view, const uint8_t* bg_valid,
                               int64_t* bg_corr, int32_t* bg_counts, int infill_border,
                               int view_surfaces, float surface_max_ratio);
int dh_reproject_surface_background(const float* bg_depth, int res, const float* grid_x, const float* grid_y,
                                    float inv_fx, float inv_fy, double fx, double fy, const float* bounds,
                                    float* zmap, float* disparity, int32_t* counts,
                                    void* workspace, size_t workspace_bytes, void* stream,
                                    const double* view, const uint8_t* bg_valid, int64_t* bg_corr, int32_t* bg_counts,
                                    int infill_border, int view_surfaces, float surface_max_ratio);
/* Bend edits (not in the reference, which moves an object as one rigid body and has no such mode; DESIGN.md, "Bend edits"):
 * linear-blend skinning of the point transform.  An instance carries n_bones transform rows per edit and every point of it a
 * weight per bone.  dh_reproject_bend_edits is dh_reproject_surface_edits plus
 *   n_bones     1 .. DH_MAX_BONES, for the call;
 *   xforms_host then [n_edits][n_instances][n_bones][DH_SIMILARITY_ROW] f64 (host): every row with the meaning it has above, its
 *               own scale and its own pivot, or else the mask's centroid;
 *   bone_w      [n_edits][n_pts][n_bones] f32 on the DEVICE, 16-byte aligned, by point-list position (instance after instance).
 * With X_b = the point under row b (the arithmetic of the entries above, unchanged), the point goes to the f64 sum, not
 * contracted, over b ascending and only over the bones with w_b != 0: acc = w_b0 * X_b0 for the first such bone, then
 * acc = acc + w_b * X_b, per component.  A point whose weights are all 0 takes bone 0 with weight 1.  The view row, the
 * projection, the clamp or discard, the stored vertices of footprints and view surfaces and the z key act on acc as they act
 * on (X, Y, Z) above.  So weights (1, 0, ..) everywhere give the bits of the call without bones.  A donor instance may have
 * bones like any other.  Plain linear-blend skinning: not volume preserving.
 * The entry never reads bone_w on the host.  The weights are the CALLER's to validate: any finite weights give the weighted
 * sum as written, with no normalisation (weights that do not sum to 1 scale the point about the camera centre).
 * n_bones = 1 with bone_w = NULL is dh_reproject_surface_edits launch for launch and byte for byte: that entry is this call.
 * Workspace: dh_reproject_bend_ws_bytes = dh_reproject_surface_ws_bytes at footprints = 0, n_bones = 1; more bones grow it only
 * by the device copy of the extra rows, n_edits * n_instances * (n_bones - 1) * DH_SIMILARITY_ROW doubles (rounded up to the
 * arena's alignment).  footprints = 1 (never with view_surfaces = 1) adds what footprints add to the instance query, so the one
 * query sizes every call of this entry.
 * DH_ERR_ARG before any launch, outputs untouched, beyond what that entry refuses: n_bones outside 1 .. DH_MAX_BONES; n_bones
 * > 1 with a null bone_w; a bone_w that is not 16-byte aligned; any of the n_edits * n_instances * n_bones rows malformed. */
#define DH_MAX_BONES 4
int dh_reproject_bend_ws_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances,
                               int view_surfaces, int footprints, int n_bones, size_t* bytes);
int dh_reproject_bend_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg,
                            int n_objects, const int32_t* obj_start, int res, const float* grid_x,
                            const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                            int n_edits, const double* xforms_host, const float* bounds,
                            float* zmap, uint8_t* raw_mask, uint8_t* clean_mask, float* disparity,
                            uint8_t* vis, int32_t* target_xy, int64_t* corr, int32_t* counts,
                            void* workspace, size_t workspace_bytes, void* stream,
                            int footprints, float max_ratio, int corr_capacity,
                            int n_instances, const int32_t* inst_obj, uint8_t* corr_inst,
                            const float* donor_depth, int n_host_objects,
                            const double* views, const uint8_t* has_view, const uint8_t* bg_valid,
                            int64_t* bg_corr, int32_t* bg_counts, int infill_border,
                            int view_surfaces, float surface_max_ratio, int n_bones, const float* bone_w);
/* THE CALL of the re-projection: one argument record.  Every dh_reproject_* entry and every *_workspace_bytes / *_ws_bytes query
 * above is this record with some members filled and the rest zero (csrc/reproject_compat.cpp); a member has the meaning, the
 * type, the place (host / device) and the refusals stated at the entry that introduced it.  ZERO MEANS OFF: a record that is
 * zero beyond the members of dh_reproject_object_edits' call (with similarity rows) is that call.
 *   struct_bytes      sizeof(dh_reproject_args); anything else is DH_ERR_ARG before any other member is read
 *   n_fg              > 0: foreground points of fg_pix.  0: the call WITHOUT a foreground point (dh_reproject_surface_background):
 *                     n_edits = 1, the view row is read when has_view[0] != 0; of the tables, the transform rows and the
 *                     foreground outputs nothing is read or written
 *   n_instances, inst_obj   inst_obj = NULL with n_instances = 0: the identity table (instance n draws mask n) on the workspace
 *                     layout of dh_reproject_footprint_edits; else the table of dh_reproject_instance_edits
 *   n_bones           0 or 1: no bones (bone_w is not read); else as dh_reproject_bend_edits
 *   n_donor_objects   the trailing masks that draw from donor_depth (0 = no donor): n_objects - n_host_objects of the donor entry
 *   xforms_host       [n_edits][n_instances or n_objects][max(n_bones, 1)][DH_SIMILARITY_ROW] f64, host
 * dh_reproject_workspace answers the workspace of the call the record describes.  It reads the sizes, the settings and the host
 * arrays obj_start, inst_obj (both given: n_pts is summed over the instances; else n_pts = n_fg) and has_view (NULL = no view),
 * no other pointer, and carves as dh_reproject does; *bytes is written only on DH_OK. */
typedef struct dh_reproject_args {
  uint32_t struct_bytes;
  int32_t res, n_fg, n_objects, n_edits, n_instances, n_bones, corr_capacity;
  int32_t footprints, n_donor_objects, infill_border, view_surfaces;
  float max_ratio, surface_max_ratio;
  float inv_fx, inv_fy;
  double fx, fy;
  /* device inputs */
  const float *depth, *bg_depth;
  const int32_t* fg_pix;
  const float *grid_x, *grid_y, *bounds, *donor_depth;
  const uint8_t* bg_valid;
  const float* bone_w;
  /* host inputs */
  const int32_t *obj_start, *inst_obj;
  const double *xforms_host, *views;
  const uint8_t* has_view;
  /* device outputs */
  float* zmap;
  uint8_t *raw_mask, *clean_mask;
  float* disparity;
  uint8_t* vis;
  int32_t* target_xy;
  int64_t* corr;
  uint8_t* corr_inst;
  int32_t* counts;
  int64_t* bg_corr;
  int32_t* bg_counts;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
} dh_reproject_args;
int dh_reproject(const dh_reproject_args* a);
int dh_reproject_workspace(const dh_reproject_args* a, size_t* bytes);
/* unprojected points only (depth_to_world_coords), [res*res][3] f32 */
int dh_unproject(const float* depth, int res, const float* grid_x, const float* grid_y,
                 float inv_fx, float inv_fy, float* points, void* stream);
/* masked centroid with NumPy's sequential float32 accumulation order (f32[3]) */
int dh_masked_centroid(const float* depth, const int32_t* fg_pix, int n_fg, int res,
                       const float* grid_x, const float* grid_y, float inv_fx, float inv_fy,
                       float* centroid, void* stream);

/* Laplacian depth blend of DiffusionHandles.set_foreground (diffusion_handles.py:90-111,
 * utils.solve_laplacian_depth utils.py:49-102): inside binary_dilation(fg_mask, dilate_iters) (cross
 * element) solve 4x - sum(masked nbrs) = sum(known depth nbrs) - laplacian(bg_depth); elsewhere copy depth.
 * counts[4] i32: {_, _, n_unknown, cg_iterations}. */
int dh_laplacian_blend_workspace_bytes(int res, size_t* bytes);
int dh_laplacian_blend(const float* depth, const float* bg_depth, const uint8_t* fg_mask, int res,
                       int dilate_iters, float* out, int32_t* counts, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The blend with the in-fill border (above): infill_border = 1 (reflect) solves deg x - sum(masked nbrs) = sum(known depth
 * nbrs) - laplacian(bg_depth) with deg the number of in-image neighbours and the Laplacian of bg_depth under replicate padding
 * (scipy.ndimage.convolve(mode="nearest")), so depth == bg_depth around the mask still gives out == bg_depth inside.
 * dh_laplacian_blend is the infill_border = 0 call.  Same workspace (dh_laplacian_blend_workspace_bytes: it does not grow).
 * DH_ERR_ARG before any launch, outputs untouched: infill_border other than 0 or 1. */
int dh_laplacian_blend_border(const float* depth, const float* bg_depth, const uint8_t* fg_mask, int res,
                              int dilate_iters, float* out, int32_t* counts, void* workspace,
                              size_t workspace_bytes, void* stream, int infill_border);

/* --------------------------------------------------------------------------------------
 * Correspondences -> grid x grid cell index lists.  Replaces
 * GuidedStableDiffuser.process_correspondences (guided_stable_diffuser.py:490-584),
 * including scipy.ndimage.binary_erosion (cross element, border 0).
 *   corr [n][4] i64 (ox, oy, tx, ty) in pixels.
 *   pairs [n][2] i32 (orig cell id, target cell id), first counts[0] valid, order kept
 *   bg_lists [3][grid*grid] i32 cell ids (row-major nonzero order) of
 *            {both, orig, trans} background masks; counts[1..3] = their lengths
 *   bg_masks [3][grid*grid] u8
 *   counts [4] i32
 * ------------------------------------------------------------------------------------ */
int dh_cells_workspace_bytes(int n, int grid, size_t* bytes);
int dh_cells_from_correspondences(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                  int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* Object removal (not in the reference; DESIGN.md, "Object removal"): dh_cells_from_correspondences with
 * vacated [img_res][img_res] u8 (may be NULL), non-zero on the pixels of the objects an edit deletes.  A cell that holds a
 * vacated pixel is cleared from the ORIGINAL-background mask, as if a kept correspondence started in it, BEFORE the erosion;
 * the transformed-background mask and the pairs do not see it, both = orig & trans as before.  n = 0 with an image is the
 * pure removal.  vacated NULL (and an all-zero image) is dh_cells_from_correspondences in every output byte, which is this
 * entry's NULL call; the workspace is dh_cells_workspace_bytes'.  DH_ERR_ARG before any launch, outputs untouched. */
int dh_cells_from_correspondences_vacated(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                          int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                          void* workspace, size_t workspace_bytes, void* stream,
                                          const uint8_t* vacated);
/* Object insertion (not in the reference; DESIGN.md, "Object insertion"): the _vacated entry with row_donor [n] u8 on the
 * device (may be NULL), non-zero on the correspondence rows whose source pixel lies in a donor image.  Such a row forms its
 * pair and clears its target cell from the transformed-background mask like any row, and does NOT clear a cell of the
 * original-background mask: nothing of the host started there.  NULL (and an all-zero array) is the _vacated entry in every
 * output byte, which is this entry's NULL call; same workspace, same refusals. */
int dh_cells_from_correspondences_donor(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                        int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                        void* workspace, size_t workspace_bytes, void* stream,
                                        const uint8_t* vacated, const uint8_t* row_donor);
/* Camera moves (not in the reference; DESIGN.md, "Camera moves"): the _donor entry with row_kind [n] u8 on the device (may be
 * NULL) in place of row_donor: 0 = a host row, 1 = a donor row, 2 = a BACKGROUND row of a camera move, which forms its pair and
 * clears neither mask -- the background stays background at both of its ends, so the global_avg term keeps its two cell lists.
 * (Any other value is read as 1.)  NULL and kinds {0, 1} are the _donor entry in every output byte, which is this entry's call
 * with those kinds; same workspace, same refusals. */
int dh_cells_from_correspondences_rows(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                       int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                       void* workspace, size_t workspace_bytes, void* stream,
                                       const uint8_t* vacated, const uint8_t* row_kind);

/* Keep map of the background lock: keep [s][s] f32, 0 inside the region an edit touches, 1 far from it, a ramp between.
 * A latent cell (res / s pixels square) is a REGION cell if one of its pixels is non-zero in mask or release (u8 [res][res],
 * either may be NULL), or if it holds the source pixel of a correspondence, or its target pixel when 0 <= tx, ty < res
 * (corr [n][4] i64 (ox, oy, tx, ty), n may be 0).  d = Chebyshev distance in cells to the nearest region cell, searched
 * within dilate + feather + 1 cells (the window is clipped by the border): keep = 0 for d <= dilate, else
 * min(1, float(d - dilate) / float(feather + 1)) by one f32 division, 1 where the window holds no region cell (an empty
 * region: all ones).  workspace: s * s bytes.  A memset and at most three launches, nothing returns to the host.
 * DH_ERR_ARG before any launch, outputs untouched: dilate < 0, feather < 0, dilate + feather > 31, res % s != 0. */
int dh_keep_map(const int64_t* corr, int n, const uint8_t* mask, const uint8_t* release, int res, int s, int dilate,
                int feather, float* keep, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------
 * depth_transform_mode = 'mesh' (depth_transform.py:91-195 + depth_to_mesh :30-71 + the pytorch3d
 * renderer outputs 'world_position' / 'flat_vertex_color'): per-pixel-quad triangulation of the
 * background depth and of the rigidly moved foreground depth (transform_points :438-458, float32),
 * nearest-z rasterisation with back-face culling, blur_radius coverage, perspective-correct clipped
 * barycentrics.  pytorch3d is not in the reference tree: parity unpinned (oracle/mesh_ref.py restates
 * the published rule; validated against the point z-buffer on smooth depth).
 *   grid   [res] f32 = linspace(-1,1,res), lin01 [res] f32 = linspace(0,1,res) (host torch values)
 *   xform  [11] f32 host: unit axis x3, cos, sin, translation x3, centroid of the masked points x3
 *   bounds NULL or device {lo, hi} of the input disparity (use_input_depth_normalization)
 * Outputs: zmap [res^2] f32 rendered depth, disparity [res^2] f32 in [0,255], fg_flag [res^2] u8,
 *          corr [<= res^2][4] i64 (src_x, src_y, tgt_x, tgt_y) in row-major target order,
 *          counts[0] = number of correspondences.
 * ------------------------------------------------------------------------------------ */
int dh_mesh_workspace_bytes(int res, size_t* bytes);
int dh_mesh_reproject(const float* depth, const float* bg_depth, const uint8_t* fg_mask, int res,
                      const float* grid, const float* lin01, float inv_f, float f, const float* xform,
                      const float* bounds, float blur_radius, float* zmap, float* disparity,
                      uint8_t* fg_flag, int64_t* corr, int32_t* counts, void* workspace,
                      size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------
 * Guidance energy (losses.py:4-84) on channels-last maps [h][w][C].
 * One call evaluates, for ONE activation layer,
 *     loss = fg_w * fg_term + bg_w * bg_term
 * and writes d(loss * grad_scale)/d(cur) for every element (no accumulation, no atomics).
 * cur/orig: [hw_in][C] in `dtype`; when hw_in != grid*grid the maps are bilinearly resized
 * (align_corners=False) to grid x grid first and the gradient is carried back.
 * bg_mode: 0 = global_avg, 1 = local_avg.  patch: fg/bg pooling window (odd, >=1).
 * pairs/bg lists as produced by dh_cells_from_correspondences (device).
 * loss_out: f32[3] = {loss, fg_term, bg_term}.  grad: same shape as cur, in `grad_dtype`.
 * ------------------------------------------------------------------------------------ */
int dh_energy_workspace_bytes(int C, int grid, int n_pairs, size_t* bytes);
int dh_energy_fwd_bwd(const void* cur, const void* orig, int dtype, int C, int h_in, int w_in, int grid,
                      const int32_t* pairs, int n_pairs,
                      const int32_t* bg_both, int n_bg_both,
                      const int32_t* bg_orig, int n_bg_orig,
                      const int32_t* bg_trans, int n_bg_trans,
                      float fg_w, float bg_w, int fg_patch, int bg_patch, int bg_mode,
                      float grad_scale, float* loss_out, void* grad, int grad_dtype,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Planned form of the same evaluation for the default configuration (maps already at the cell grid,
 * fg_patch 1, bg 'global_avg' -- config/default.yaml:5-9), 16-bit activations.  The correspondences of an
 * edit are fixed over its 38 x 3 evaluations, so the target-cell -> (distinct source cell, multiplicity) CSR and the
 * transformed-background flags are built ONCE (dh_energy_plan_build) and every evaluation is three kernels
 * that read the activations once in their own dtype.  Same arithmetic per element as dh_energy_fwd_bwd:
 * the gradient is bit-identical.  loss_out may be NULL (the guided loop only needs the gradient). */
int dh_energy_plan_bytes(int grid, int n_pairs, size_t* bytes);
int dh_energy_plan_build(const int32_t* pairs, int n_pairs, const int32_t* bg_trans, int n_bg_trans, int grid,
                         void* plan, size_t plan_bytes, void* stream);
int dh_energy_planned_workspace_bytes(int C, int grid, size_t* bytes);
int dh_energy_fwd_bwd_planned(const void* cur, const void* orig, int dtype, int C, int grid,
                              const void* plan, size_t plan_bytes, int n_pairs,
                              const int32_t* bg_orig, int n_bg_orig, const int32_t* bg_trans, int n_bg_trans,
                              float fg_w, float bg_w, float grad_scale, float* loss_out, void* grad,
                              int grad_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* The planned evaluation for K <= 16 items (edits of one image or of different images) in ONE launch pair: one
 * background column-sum launch (grid z = 2 K) and one gradient launch (grid y = item), plus one loss launch only when an
 * item has a loss_out.  Nothing is shared between items: every field is what dh_energy_fwd_bwd_planned takes for that
 * item (cur / orig / grad are unrelated pointers; n_pairs = 0, empty background lists, zero weights allowed); dtype, C,
 * grid and grad_dtype are common.  The item table reaches the kernels by value in their arguments: no device allocation,
 * copy or synchronisation.  Per element the arithmetic and its order are those of the single call: the gradient and the
 * loss values of item e are bit-identical to dh_energy_fwd_bwd_planned's.  K > 16 is an error (never split). */
typedef struct dh_energy_item {
  const void* cur;
  const void* orig;
  const void* plan;
  size_t plan_bytes;
  const int32_t* bg_orig;
  const int32_t* bg_trans;
  float* loss_out;            /* NULL: no loss values for this item */
  void* grad;
  int n_pairs, n_bg_orig, n_bg_trans;
  float fg_w, bg_w, grad_scale;
} dh_energy_item;
int dh_energy_planned_batch_workspace_bytes(int C, int grid, int n_items, size_t* bytes);
int dh_energy_fwd_bwd_planned_batch(const dh_energy_item* items, int n_items, int dtype, int C, int grid,
                                    int grad_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* A weight per object for the foreground term of multi-object edits (extends dh_energy_plan_build /
 * dh_energy_fwd_bwd_planned / dh_energy_fwd_bwd_planned_batch; same configuration, dtypes and workspaces).  With N_m pairs
 * of object m and weights w_m >= 0, omega_m = w_m / (sum of w_j over the objects with N_j > 0) and
 *     fg_term = sum_m omega_m * mean_c mean_{n in object m} | A_orig[c, o_n] - A_cur[c, t_n] |
 * so the coefficient of a pair of object m is fg_w * omega_m / (C N_m) instead of fg_w / (C N).  The background term and the
 * background lists are unchanged (the union's).  pair_obj: the 0-based object of every pair (device, one byte each);
 * weights / counts: n_objects host values, counts[m] = N_m (they must add up to n_pairs).  Errors, before any launch:
 * n_objects outside 1..8, a negative or non-finite weight, no positive weight among the objects that have pairs
 * (n_pairs = 0 is allowed: no foreground term).  A plan built here is only valid for the two _objects evaluations below
 * (it needs dh_energy_plan_objects_bytes); they take what their unweighted forms take, workspaces included
 * (dh_energy_planned_workspace_bytes for the single call).  One launch pair, one writer per gradient element, a fixed
 * summation order (objects ascending): bit-reproducible, and the batch is bit-identical per item to the single call. */
int dh_energy_plan_objects_bytes(int grid, int n_pairs, size_t* bytes);
int dh_energy_plan_build_objects(const int32_t* pairs, const uint8_t* pair_obj, int n_pairs, const int32_t* bg_trans,
                                 int n_bg_trans, int grid, int n_objects, const float* weights, const int32_t* counts,
                                 void* plan, size_t plan_bytes, void* stream);
int dh_energy_fwd_bwd_planned_objects(const void* cur, const void* orig, int dtype, int C, int grid,
                                      const void* plan, size_t plan_bytes, int n_pairs,
                                      const int32_t* bg_orig, int n_bg_orig, const int32_t* bg_trans, int n_bg_trans,
                                      float fg_w, float bg_w, float grad_scale, float* loss_out, void* grad,
                                      int grad_dtype, void* workspace, size_t workspace_bytes, void* stream);
int dh_energy_planned_objects_batch_workspace_bytes(int C, int grid, int n_items, size_t* bytes);
int dh_energy_fwd_bwd_planned_objects_batch(const dh_energy_item* items, int n_items, int dtype, int C, int grid,
                                            int grad_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* K <= 16 items of which some carry a weighted plan (dh_energy_plan_build_objects) and some a plain one
 * (dh_energy_plan_build), in ONE launch pair: the column-sum and loss launches of dh_energy_fwd_bwd_planned_batch and one
 * gradient launch whose workgroups take the weighted or the unweighted arithmetic by their item.  weighted: n_items host
 * bytes, non-zero where item e's plan buffer is a weighted plan; read on the host only (the kernels receive one object-block
 * pointer per item by value, null for an unweighted item): no device allocation, copy or synchronisation.  The workspace is
 * dh_energy_planned_batch_workspace_bytes'.  Item e's gradient and loss values are bit-identical to
 * dh_energy_fwd_bwd_planned_objects' (weighted) or dh_energy_fwd_bwd_planned's (unweighted) on the same inputs; any mix is
 * allowed, all of one kind included.  Errors, before any launch: K outside 1..16 (never split), a plan buffer smaller than
 * its kind needs (so a weighted flag on a plain plan's buffer is refused). */
int dh_energy_fwd_bwd_planned_mixed_batch(const dh_energy_item* items, const uint8_t* weighted, int n_items, int dtype, int C,
                                          int grid, int grad_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Donor objects (not in the reference; DESIGN.md, "Object insertion"): dh_energy_fwd_bwd_planned_objects[_batch] for edits
 * that bring in objects of another image.  donor: that image's activations, [grid * grid][C] channels-last in the dtype of
 * orig; donor_objects: bit m set = the foreground term of a pair of object m reads A_donor[c, o_n] in place of A_orig[c, o_n].
 * The plan is dh_energy_plan_build_objects', unchanged; the background term and its lists read orig.  One writer per gradient
 * element, objects ascending, no atomics.  donor_objects = 0 (donor may then be NULL) launches and computes what the _objects
 * entry does; donor == orig with any bits gives its bytes too.  The batch takes K <= 16 weighted items, each with its donor;
 * item e is bit-identical to the single call.  Workspaces are the _objects entries'.  Refused before any launch: a bit at
 * or above 8 (the most objects a plan holds; the plan's own count lives on the device, so the caller checks bits against
 * it), bits set with a null donor, and what the _objects entries refuse. */
int dh_energy_fwd_bwd_planned_donor(const void* cur, const void* orig, int dtype, int C, int grid,
                                    const void* plan, size_t plan_bytes, int n_pairs,
                                    const int32_t* bg_orig, int n_bg_orig, const int32_t* bg_trans, int n_bg_trans,
                                    float fg_w, float bg_w, float grad_scale, float* loss_out, void* grad,
                                    int grad_dtype, void* workspace, size_t workspace_bytes, void* stream,
                                    const void* donor, uint32_t donor_objects);
typedef struct dh_energy_donor_item {
  dh_energy_item item;
  const void* donor;          /* NULL allowed with donor_objects = 0 */
  uint32_t donor_objects;
} dh_energy_donor_item;
int dh_energy_fwd_bwd_planned_donor_batch(const dh_energy_donor_item* items, int n_items, int dtype, int C, int grid,
                                          int grad_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------
 * SD-2-depth U-Net engine (model/unet_2d_condition.py:809-1198 and the block files it
 * calls): forward with the three decoder activation captures, and the backward pass to the
 * input sample / to the text embedding.  Channels-last 16-bit activations, f32 accumulate.
 * ------------------------------------------------------------------------------------ */
typedef struct dh_unet dh_unet;

typedef struct dh_unet_config {
  int in_channels;            /* 5 */
  int out_channels;           /* 4 */
  int n_levels;               /* 4 */
  int block_out_channels[4];  /* 320 640 1280 1280 */
  int layers_per_block;       /* 2 */
  int heads[4];               /* 5 10 20 20 (head dim must be 64) */
  int cross_attention_dim;    /* 1024 */
  int norm_groups;            /* 32 */
  int sample_size;            /* 64 (latent H = W) */
  int text_len;               /* 77 */
  int max_batch;              /* largest batch a forward will see */
  int dtype;                  /* DH_DTYPE_F16 or DH_DTYPE_BF16 */
  int max_diff_batch;         /* largest batch of a forward that is SAVED for a backward pass (0 = max_batch).  A forward nobody
                               * differentiates (the CFG pass at twice the edit batch, initial inference, DDIM inversion) does not keep
                               * a slot per tensor: its tensors share the activation arena by liveness, so only this batch sizes the
                               * activation / gradient arenas (batched edits: max_batch = 2 K, max_diff_batch = K) */
} dh_unet_config;

int dh_unet_create(const dh_unet_config* cfg, dh_unet** out);
/* A second engine on the SAME weights: `parent`'s 16-bit weight arena and f32 parameter arena are used read-only (3.4 GB at
 * fp16, resident once), everything a pass writes -- activations, gradients, split-K slabs, statistics, I/O buffers, graphs --
 * is private (dh_unet_workspace_bytes).  Two such engines driven on two HIP streams run two independent edits concurrently in
 * one process (the reference runs one process per device and one edit at a time, webapp/start_webapps_in_tmux.sh:21-43; a
 * single edit's passes leave most of the chip idle at any instant).  Load every parameter into `parent` BEFORE sharing: the
 * folded LayerNorm weights are finalised here (on `stream`, synchronised), and dh_unet_load_param on a shared engine is an
 * error.  `parent` must outlive the engines that share its weights.  max_batch <= 0: the parent's. */
int dh_unet_create_shared(dh_unet* parent, int max_batch, void* stream, dh_unet** out);
void dh_unet_destroy(dh_unet* u);
/* parameter table: diffusers state-dict names, torch shapes */
int dh_unet_num_params(const dh_unet* u);
int dh_unet_param_info(const dh_unet* u, int i, const char** name, int* ndim, int64_t* shape4);
/* upload parameter i from a DEVICE f32 tensor in torch layout (conv: [Cout,Cin,kh,kw]) */
int dh_unet_load_param(dh_unet* u, int i, const float* src, void* stream);
size_t dh_unet_weight_bytes(const dh_unet* u);
size_t dh_unet_workspace_bytes(const dh_unet* u);

/* forward.  sample [B][H][W][Cin] f32 channels-last; timestep host float; text [B][L][D] f32.
 * eps_out [B][H][W][Cout] f32.  act_out[3] (may be NULL): [B][h][w][C] in engine dtype.
 * save_for_backward != 0 keeps what dh_unet_backward needs (one saved pass at a time). */
int dh_unet_forward(dh_unet* u, const float* sample, float timestep, const float* text, int batch,
                    int save_for_backward, float* eps_out, void* const* act_out, void* stream);
/* backward of the LAST saved forward.  d_act[3]: gradients w.r.t. the three captured
 * activations (engine dtype, may be NULL each); d_eps: gradient w.r.t. eps (f32, may be
 * NULL).  Outputs (either may be NULL): d_sample [B][H][W][Cin] f32, d_text [B][L][D] f32. */
int dh_unet_backward(dh_unet* u, void* const* d_act, const float* d_eps, float* d_sample, float* d_text,
                     void* stream);
/* The engine's own input / output buffers (fixed addresses: its passes replay as hipGraphs).  A caller that writes its
 * inputs there (dh_pack_sample) and hands the SAME pointers to dh_unet_forward / dh_unet_backward, or lets the energy kernels
 * read the captured activations and write their cotangents in place, saves the device-to-device copies either side of a pass
 * (guided_stable_diffuser.py:397-434 builds `torch.cat([latents, depth])` and reads `unet_output[4..6]` every iteration).
 * Every buffer holds max_batch items (DH_IO_ACT_GRAD: max_diff_batch); contents are valid until the next pass that writes them.
 *   which: DH_IO_SAMPLE [B][H][W][Cin] f32 | DH_IO_TEXT [B][L][D] f32 | DH_IO_EPS [B][H][W][Cout] f32 (eps out / d_eps in) |
 *          DH_IO_ACT index 0..2 [B][h][w][C] engine dtype | DH_IO_ACT_GRAD index 0..2 (cotangent of that activation) |
 *          DH_IO_DSAMPLE [B][H][W][Cin] f32 | DH_IO_DTEXT [B][L][D] f32 */
#define DH_IO_SAMPLE 0
#define DH_IO_TEXT 1
#define DH_IO_EPS 2
#define DH_IO_ACT 3
#define DH_IO_ACT_GRAD 4
#define DH_IO_DSAMPLE 5
#define DH_IO_DTEXT 6
int dh_unet_io_ptr(dh_unet* u, int which, int index, void** ptr, size_t* bytes);
/* HIP-event bracket around every launch of the MFMA implicit-GEMM kernel (k_gemm) between begin
 * and end: total milliseconds, number of launches and their algorithmic flops (2*M*N*K).
 * Used by bench.py for the roofline figure; not on the product path. */
int dh_gemm_profile_begin(void);
int dh_gemm_profile_end(double* ms_total, int64_t* launches, double* flops);
/* ALGORITHMIC HBM bytes of the launches bracketed since the last dh_gemm_profile_begin (valid after _end as well): every
 * operand once in its 16-bit storage type -- the A source (dense rows [M][K]; for a convolution the source image
 * [B][Hin][Win][Cin], not its im2col view), the weights [N][K], the output [M][N] and the residual [M][N] when there is one
 * (GEGLU epilogues: the [M][N/2] activation on top, or the [M][2N] pre-activations read and their gradient written in place of
 * the output).  Split-K slabs, im2col tap re-reads and per-XCD re-fetches are NOT in it: `roofline.traffic` (PMC) divided by
 * this figure is the wasted-traffic ratio.  Not on the product path. */
int dh_gemm_profile_bytes(double* bytes);
/* per-kernel-class accumulated launch counts / algorithmic flops of the last forward */
/* Names the text embedding of the following dh_unet_forward calls (0 = unnamed, the default).  The K|V projections of every
 * cross-attention layer depend on the text only; a forward that finds those of the same key, batch and stream already in the
 * engine skips recomputing them.  The caller must change the key whenever the text tensor's content changes
 * (guided_stable_diffuser.py:404-410: the prompt embedding is constant over the optimisation passes of an edit). */
int dh_unet_set_text_key(dh_unet* u, unsigned long long key);
int dh_unet_stats(const dh_unet* u, double* flops_fwd, double* flops_bwd, int64_t* launches);

/* --------------------------------------------------------------------------------------
 * Loop arithmetic (f32 latents, channels-last [B][H][W][4]).
 * ------------------------------------------------------------------------------------ */
/* eps = eps_u + scale*(eps_c - eps_u); x <- sqrt(a_prev)*(x - sqrt(1-a_t) eps)/sqrt(a_t) +
 * sqrt(1-a_prev) eps.   DDIMScheduler.step, eta 0 (guided_stable_diffuser.py:468-474) and
 * prev_step/next_step (stable_null_inverter.py:25-43).  eps_u may be NULL (no CFG). */
int dh_ddim_cfg_step(float* x_out, const float* x, const float* eps_u, const float* eps_c, float scale,
                     float alpha_t, float alpha_prev, int n, void* stream);
/* x_out = x - lr * g / grad_scale                         guided_stable_diffuser.py:434 */
int dh_latent_update(float* x_out, const float* x, const float* g, float lr, float grad_scale, int n,
                     void* stream);
/* the same with g read out of a wider gradient: g [pixels][g_channels], the first `channels` of every pixel (the latent
 * channels of d(sample) = d(cat[latents, depth])) */
int dh_latent_update_strided(float* x_out, const float* x, const float* g, int g_channels, int channels, float lr,
                             float grad_scale, int pixels, void* stream);
/* Guarded forms for the 'auto' guidance scale (conf.guided_diffuser.grad_scale; the latent update of
 * guided_stable_diffuser.py:434 and the DDIM step of :468-474).  status: int[edits][4] per edit = {kinds seen (bit 0: the
 * backward overflowed and the update was held, bit 1: a latent element is not finite after the DDIM step), number of held
 * updates, code of the first failure ((t_idx + 1) << 16 | (iteration & 0xff) << 8 | kind, 0 = none), 0}; the caller zeroes it.
 * dh_latent_update_guarded: one workgroup per edit, edits of `pixels` x `channels` (at most 48 K elements) read out of g
 * [edits][pixels][g_channels]; per edit, x_out = x - (lr / S_e) g if every element of its slice is finite, else x_out = x
 * and the status records the held update.  S_e = scale_table[e * table_stride + table_index], a power of two; with S_e =
 * grad_scale the result is bit-identical to dh_latent_update_strided.  gmax (may be NULL): [edits] max |g| / S_e (NaN when held). */
int dh_latent_update_guarded(float* x_out, const float* x, const float* g, int g_channels, int channels, float lr, int pixels,
                             int edits, const float* scale_table, int table_stride, int table_index, int* status, float* gmax,
                             int t_idx, int iteration, void* stream);
/* dh_ddim_cfg_step, plus bit 1 of status[i / n_edit] where output element i is not finite (n_edit: elements per edit) */
int dh_ddim_cfg_step_flagged(float* x_out, const float* x, const float* eps_u, const float* eps_c, float scale, float alpha_t,
                             float alpha_prev, int n, int n_edit, int* status, int t_idx, int iteration, void* stream);
/* Background lock: dh_ddim_cfg_step for n / n_edit edits (at most 16; more is an error), each blended with its
 * reconstruction outside the region its edit touches.  items[e] = {keep [n_edit / channels] f32 (one value per latent cell, from
 * dh_keep_map), ref [n_edit] f32 (the reconstruction's latent after THIS step, channels-last)}; keep == NULL: edit e is not
 * locked.  With o = dh_ddim_cfg_step's value: x_out = o where keep == 0 and for an unlocked edit (bit-identical to
 * dh_ddim_cfg_step), x_out = ref where keep == 1, x_out = o + keep (ref - o) in between.  status may be NULL (static
 * guidance scale); otherwise bit 1 of status[e] is set as dh_ddim_cfg_step_flagged sets it, judged on o BEFORE the blend (a
 * locked cell does not hide a step that went bad).  One launch; the table travels by value in the kernel arguments. */
typedef struct dh_lock_item {
  const float* keep;          /* NULL: not locked */
  const float* ref;
} dh_lock_item;
int dh_ddim_cfg_step_locked(float* x_out, const float* x, const float* eps_u, const float* eps_c, float scale, float alpha_t,
                            float alpha_prev, int n, int n_edit, int channels, const dh_lock_item* items, int n_items,
                            int* status, int t_idx, int iteration, void* stream);
/* dst[b][p][:] = concat(latent[b or 0][p][0:latent_channels], depth[b or 0][p][0:depth_channels]) for b < batch: the U-Net
 * input `torch.cat([latents (x batch), depth (x batch)], dim=1)` (guided_stable_diffuser.py:400-401, 451-455) in one launch.
 * latent_batch / depth_batch divide batch: item b reads latent[b mod latent_batch] (1 = broadcast, batch = one each, K of 2K =
 * the K edits repeated for the two halves of the CFG pass); depth may be NULL (use_depth false). */
int dh_pack_sample(float* dst, const float* latent, int latent_batch, int latent_channels, const float* depth,
                   int depth_batch, int depth_channels, int batch, int pixels, void* stream);
/* Adam step on the null-text embedding (torch defaults; stable_null_inverter.py:143-155) */
int dh_adam_step(float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                 float eps, int step, int n, void* stream);
/* mse(rec, target) and d mse / d rec                        stable_null_inverter.py:152 */
int dh_mse_fwd_bwd(const float* rec, const float* target, int n, float* loss_out, float* d_rec,
                   void* stream);
/* The same loss, and the cotangent that seeds the engine's backward of a null-text inner step
 * (stable_null_inverter.py:150-154: loss.backward() through prev_step and the CFG combine down to eps_uncond):
 *   d_eps = (d mse / d rec) * k * S,   k = d rec / d eps_uncond (a scalar of the timestep),
 * S = the power of two that brings max |d_eps| into (amp / 2, amp] (amp <= 0: S = 1), written to scale_out[0] (device).
 * The 16-bit backward is linear in its cotangent: S only keeps it out of the fp16 subnormal range and is divided out
 * again by dh_adam_step_scaled. */
int dh_mse_cotangent(const float* rec, const float* target, int n, float k, float amp, float* loss_out,
                     float* d_eps, float* scale_out, void* stream);
/* dh_adam_step on g / g_scale[0] (g_scale: device scalar, the S of dh_mse_cotangent) */
int dh_adam_step_scaled(float* p, const float* g, const float* g_scale, float* m, float* v, float lr, float beta1,
                        float beta2, float eps, int step, int n, void* stream);
/* dh_mse_cotangent for `batch` images of n elements each (rec / target / d_eps [batch][n]; loss_out / scale_out [batch]),
 * with the per-image early stop of the null-text inner loop (stable_null_inverter.py:141-158; checked after the step's Adam
 * update): an image with active[b] == 0 on entry gets d_eps = 0 and S = 1; every image gets loss_out[b];
 * updated[b] = active[b] on entry, then active[b] = active[b] && !((double)loss_out[b] < threshold).  The threshold is a double
 * compared against the f32 loss widened to double, like the host's `loss.item() < epsilon + 2e-5 i`.  batch = 1 is bit-identical
 * to dh_mse_cotangent. */
int dh_mse_cotangent_batch(const float* rec, const float* target, int batch, int n, float k, float amp, double threshold,
                           int* active, int* updated, float* loss_out, float* d_eps, float* scale_out, void* stream);
/* dh_adam_step_scaled on image b of `batch` (p / g / m / v [batch][n]) with g_scale[b], only where updated[b] != 0 (the others
 * keep parameters and moments); batch = 1 is bit-identical to dh_adam_step_scaled */
int dh_adam_step_scaled_batch(float* p, const float* g, const float* g_scale, const int* updated, float* m, float* v, float lr,
                              float beta1, float beta2, float eps, int step, int batch, int n, void* stream);

/* --------------------------------------------------------------------------------------
 * SD AutoencoderKL decoder on the engine's kernels: the decode that ends every edit
 * (guided_stable_diffuser.py:481-483 decode_latent_image, :286; stable_null_inverter.py:105 latent2image).
 * diffusers' AutoencoderKL is [ext]; parameter names are its state-dict names ("decoder.*").
 * z: [B][h][w][latent_channels] f32 channels-last, ALREADY divided by the scaling factor and passed through
 * post_quant_conv (a 4x4 matrix per pixel, host side); image: [B][8h][8w][out_channels] f32.  Forward only.
 * ------------------------------------------------------------------------------------ */
typedef struct dh_vae_decoder dh_vae_decoder;
typedef struct dh_vae_config {
  int latent_channels;        /* 4 */
  int out_channels;           /* 3 */
  int block_out_channels[4];  /* 128 256 512 512 (encoder order, as in the VAE's config.json) */
  int layers_per_block;       /* 2 (the decoder runs layers_per_block + 1 resnets per up block) */
  int norm_groups;            /* 32 */
  int latent_size;            /* 64 (latent H = W; image = 8x) */
  int dtype;                  /* DH_DTYPE_F16 or DH_DTYPE_BF16 */
} dh_vae_config;
int dh_vae_decoder_create(const dh_vae_config* cfg, dh_vae_decoder** out);
void dh_vae_decoder_destroy(dh_vae_decoder* v);
int dh_vae_decoder_num_params(const dh_vae_decoder* v);
int dh_vae_decoder_param_info(const dh_vae_decoder* v, int i, const char** name, int* ndim, int64_t* shape4);
int dh_vae_decoder_load_param(dh_vae_decoder* v, int i, const float* src, void* stream);   /* DEVICE f32, torch layout */
size_t dh_vae_decoder_bytes(const dh_vae_decoder* v);
int dh_vae_decoder_decode(dh_vae_decoder* v, const float* z, int batch, float* image, void* stream);
/* The encoder half on the same kernels (stable_null_inverter.py:72-83 image2latent: `vae.encode(image)['latent_dist'].mean`,
 * once per image).  The handle has the decoder's type and shares its parameter / destroy / bytes entry points; the state-dict
 * names are "encoder.*".  image: [B][8h][8w][out_channels] f32 channels-last in [-1, 1]; moments: [B][h][w][2 * latent_channels]
 * f32 (conv_out of the encoder: the caller applies the 1x1 quant_conv and takes the first latent_channels as the mean). */
int dh_vae_encoder_create(const dh_vae_config* cfg, dh_vae_decoder** out);
int dh_vae_encoder_encode(dh_vae_decoder* v, const float* image, int batch, float* moments, void* stream);

/* --------------------------------------------------------------------------------------
 * CLIP text tower on the engine's kernels (guided_stable_diffuser.py:96-108 `self.text_encoder(ids)[0]`,
 * stable_null_inverter.py:85-103): pre-norm transformer layers with causal attention (heads of 64), erf-GELU MLP and the
 * final LayerNorm.  transformers' CLIPTextModel is [ext]; parameter names are its state-dict names
 * ("text_model.encoder.layers.N.*", "text_model.final_layer_norm.*").  The token + position embedding lookup stays with the
 * caller: embeds [B][tokens][hidden] f32 is their sum; out [B][tokens][hidden] f32 = last_hidden_state.  Forward only.
 * ------------------------------------------------------------------------------------ */
typedef struct dh_text_encoder dh_text_encoder;
typedef struct dh_text_config {
  int hidden;        /* 1024 */
  int heads;         /* 16 (head dim 64) */
  int layers;        /* 23 */
  int intermediate;  /* 4096 */
  int max_tokens;    /* 77 */
  int max_batch;     /* prompts per call */
  float eps;         /* 1e-5 */
  int dtype;         /* DH_DTYPE_F16 or DH_DTYPE_BF16 */
} dh_text_config;
int dh_text_encoder_create(const dh_text_config* cfg, dh_text_encoder** out);
void dh_text_encoder_destroy(dh_text_encoder* e);
int dh_text_encoder_num_params(const dh_text_encoder* e);
int dh_text_encoder_param_info(const dh_text_encoder* e, int i, const char** name, int* ndim, int64_t* shape2);
int dh_text_encoder_load_param(dh_text_encoder* e, int i, const float* src, void* stream);   /* DEVICE f32, torch layout */
size_t dh_text_encoder_bytes(const dh_text_encoder* e);
int dh_text_encoder_encode(dh_text_encoder* e, const float* embeds, int batch, int tokens, float* out, void* stream);

/* --------------------------------------------------------------------------------------
 * Host-only query of the GEMM dispatch (csrc/gemm.hip: gemm_plan): which kernel, tile, K split, epilogue riders and reduce a
 * launch of this description gets.  No launch, no device needed; the description carries no pointers.  out receives 23 values:
 * pp, bm, bn, stages, wg, kg, mw, gm (0 dense, 1 stride-1 3x3, 2 generic), buf, lnf, epi (0 plain, 1 / 2 GEGLU forward / backward,
 * 3 / 4 cross-attention forward / dQ), splits, k_per_split, grid x, y, z, a_bytes, w_bytes, gn_epi (1 forward, 2 backward GroupNorm
 * statistics in the epilogue), gn_cpg, gn_S, xa, reduce (0 none, 1 plain, 2 / 3 with GroupNorm forward / backward statistics,
 * 4 with the LayerNorm backward).  tests/test_gemm_plan.py pins the table of the SD-2-depth passes.
 * ------------------------------------------------------------------------------------ */
#define DH_GEMM_Q_BIAS 0x1u
#define DH_GEMM_Q_RESIDUAL 0x2u
#define DH_GEMM_Q_ROWVEC 0x4u        /* per-image vector */
#define DH_GEMM_Q_SILU 0x8u
#define DH_GEMM_Q_LNF 0x10u          /* folded LayerNorm */
#define DH_GEMM_Q_GN_STATS 0x20u     /* GroupNorm statistics of the output wanted (gn_HW, gn_G) */
#define DH_GEMM_Q_GN_BWD 0x40u       /* ... the backward statistics: the output is dy of that GroupNorm */
#define DH_GEMM_Q_LN_BWD 0x80u       /* LayerNorm backward on the split-K reduce */
#define DH_GEMM_Q_GLU_FWD 0x100u
#define DH_GEMM_Q_GLU_BWD 0x200u     /* glub_f: columns of the GEGLU's dy (N = all) */
#define DH_GEMM_Q_XATTN_FWD 0x400u   /* cross-attention in the epilogue (xa_Nq, xa_Nk, xa_H) */
#define DH_GEMM_Q_XATTN_DQ 0x800u    /* ... its dQ */
#define DH_GEMM_Q_ALIGNED 0x1000u    /* every operand 16-byte aligned (and, by its shape, below 2 GiB) */
typedef struct dh_gemm_plan_query {
  int32_t M, N, K;
  int32_t conv;              /* 0 dense, 1 = 3x3 convolution (K = 9 Cin), 2 = input gradient of a stride-2 3x3 convolution */
  int32_t hw, stride, up;    /* conv: side of the square source image, stride 1 / 2, nearest-2x up-sampled source */
  int64_t lda, ldc;          /* 0 = the defaults: K (dense) or Cin (conv); N */
  uint64_t partial_elems;    /* f32 elements of split-K workspace */
  uint32_t flags;            /* DH_GEMM_Q_* */
  int32_t gn_HW, gn_G, glub_f, xa_Nq, xa_Nk, xa_H;
} dh_gemm_plan_query;
int dh_dbg_gemm_plan(const dh_gemm_plan_query* q, int32_t* out, int n_out);

/* --------------------------------------------------------------------------------------
 * Host-only query of the attention dispatch (csrc/attention.hip: attn_plan): which variant of the flash-attention forward (kind 0),
 * dQ (1) or dK/dV (2) kernel a launch of this description gets.  No launch, no device needed; the description carries no pointers.
 * out receives 11 values: launch (0 = a dimension is <= 0, nothing would run), ks, qw, db, grid x, y, z, block, qchunks, reduce
 * (1 = k_attn_dkv_reduce follows), scratch_used (f32 elements).  force_* and cus replace the dispatch's hooks for this query
 * (0 = leave them: no forced value, 256 compute units).  tests/test_attn_plan.py pins the table of the SD-2-depth passes.
 * dh_dbg_attn_last_launch: what this thread's last launch of `kind` passed to the device, written by the launcher from its own
 * template arguments: out[0..8] = ks, qw, db, grid x, y, z, block, qchunks, reduce.
 * ------------------------------------------------------------------------------------ */
typedef struct dh_attn_plan_query {
  int32_t kind, B, H, Nq, Nk, causal;
  uint64_t scratch_elems;    /* f32 elements of dK/dV workspace; 0 = none */
  int32_t force_ks, force_qw, force_dkv_ks, force_dkv_qw, cus;
} dh_attn_plan_query;
int dh_dbg_attn_plan(const dh_attn_plan_query* q, int32_t* out, int n_out);
int dh_dbg_attn_last_launch(int kind, int32_t* out, int n_out);

/* --------------------------------------------------------------------------------------
 * LayerNorm forward (y [rows][C], stats [rows][2] = (mean, rstd) per row; stats may be NULL) and, when dy and dx are given, its
 * backward dx = rstd (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat)) (+ add), the way the engines launch the pair: x has the
 * row pitch ldx (elements, >= C, a multiple of 8), every other operand is dense; add may be NULL or alias dx.  dtype: DH_DTYPE_F16 /
 * DH_DTYPE_BF16 for x, y, dy, add, dx; gamma, beta f32.  Refused: C % 8 != 0, C > 4096 (one wave holds a row as at most eight
 * sixteen-byte chunks per lane), a backward without stats.  tests/test_layernorm_gpu.py.
 * ------------------------------------------------------------------------------------ */
int dh_dbg_layernorm_ld(int dtype, const void* x, long ldx, const float* gamma, const float* beta, void* y, float* stats,
                        const void* dy, const void* add, void* dx, int rows, int C, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
