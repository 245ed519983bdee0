// The positional entries and workspace queries of the re-projection (include/diffhandles_hip.h): each fills a dh_reproject_args
// and calls dh_reproject / dh_reproject_workspace (geometry.hip).  Host only.  Every entry is documented in the header as the
// call it was; here it is "the record with these members", and none calls another.  A check an entry made itself, ahead of the
// shared ones, is still made here, with its text.
#include "common.h"

#include <vector>

namespace {

constexpr int MAX_OBJECTS = 8;
const uint8_t ONE = 1;

// The parameter lists: every object entry took the list of the one before it and a few more (P0: dh_reproject_object_edits',
// P1: + footprints, P2: + the instance table, P3: + the donor, P4: + the views); A0 .. A4 hand the same names on.
#define P0                                                                                                                       \
  const float *depth, const float *bg_depth, const int32_t *fg_pix, int n_fg, int n_objects, const int32_t *obj_start, int res, \
      const float *grid_x, const float *grid_y, float inv_fx, float inv_fy, double fx, double fy, int n_edits,                  \
      const double *xforms_host, const float *bounds, float *zmap, uint8_t *raw_mask, uint8_t *clean_mask, float *disparity,    \
      uint8_t *vis, int32_t *target_xy, int64_t *corr, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream
#define A0                                                                                                                       \
  depth, bg_depth, fg_pix, n_fg, n_objects, obj_start, res, grid_x, grid_y, inv_fx, inv_fy, fx, fy, n_edits, xforms_host, bounds, \
      zmap, raw_mask, clean_mask, disparity, vis, target_xy, corr, counts, workspace, workspace_bytes, stream
#define P1 P0, int footprints, float max_ratio, int corr_capacity
#define A1 A0, footprints, max_ratio, corr_capacity
#define P2 P1, int n_instances, const int32_t *inst_obj, uint8_t *corr_inst
#define A2 A1, n_instances, inst_obj, corr_inst
#define P3 P2, const float *donor_depth, int n_host_objects
#define A3 A2, donor_depth, n_host_objects
#define P4 P3, const double *views, const uint8_t *has_view, const uint8_t *bg_valid, int64_t *bg_corr, int32_t *bg_counts
#define A4 A3, views, has_view, bg_valid, bg_corr, bg_counts
// ... and the entries without a foreground point (B1: + the view row)
#define PB0                                                                                                                      \
  const float *bg_depth, int res, const float *grid_x, const float *grid_y, float inv_fx, float inv_fy, double fx, double fy,   \
      const float *bounds, float *zmap, float *disparity, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream
#define AB0 bg_depth, res, grid_x, grid_y, inv_fx, inv_fy, fx, fy, bounds, zmap, disparity, counts, workspace, workspace_bytes, stream
#define PB1 PB0, const double *view, const uint8_t *bg_valid, int64_t *bg_corr, int32_t *bg_counts
#define AB1 AB0, view, bg_valid, bg_corr, bg_counts

// A record under construction; fill_k takes the list P_k.  The positional entries never meant "off" by a zero where the record
// does, so two zeros are kept apart: an object entry with n_fg = 0 is not the call without a foreground point, and a table
// entry with no table (n_instances = 0, inst_obj = NULL) is not the identity table.  Both stay the refusals they were ("bad
// sizes", "null input").
struct Record : dh_reproject_args {
  Record() : dh_reproject_args{} { struct_bytes = sizeof(dh_reproject_args); }
  Record& fill0(P0) {
    this->depth = depth, this->bg_depth = bg_depth, this->fg_pix = fg_pix, this->n_fg = n_fg != 0 ? n_fg : -1;
    this->n_objects = n_objects, this->obj_start = obj_start, this->res = res, this->grid_x = grid_x, this->grid_y = grid_y;
    this->inv_fx = inv_fx, this->inv_fy = inv_fy, this->fx = fx, this->fy = fy, this->n_edits = n_edits;
    this->xforms_host = xforms_host, this->bounds = bounds, this->zmap = zmap, this->raw_mask = raw_mask;
    this->clean_mask = clean_mask, this->disparity = disparity, this->vis = vis, this->target_xy = target_xy;
    this->corr = corr, this->counts = counts, this->workspace = workspace, this->workspace_bytes = workspace_bytes;
    this->stream = stream, this->corr_capacity = n_fg;          // (the entries without a capacity: one row per point)
    return *this;
  }
  Record& fill1(P1) {
    this->footprints = footprints, this->max_ratio = max_ratio;
    return fill0(A0).capacity(corr_capacity);
  }
  Record& capacity(int corr_capacity) { return this->corr_capacity = corr_capacity, *this; }
  Record& fill2(P2) {
    this->n_instances = n_instances != 0 || inst_obj ? n_instances : -1, this->inst_obj = inst_obj, this->corr_inst = corr_inst;
    return fill1(A1);
  }
  Record& fill3(P3) {
    this->donor_depth = donor_depth, this->n_donor_objects = n_objects - n_host_objects;
    return fill2(A2);
  }
  Record& fill4(P4) {
    this->views = views, this->has_view = has_view, this->bg_valid = bg_valid, this->bg_corr = bg_corr, this->bg_counts = bg_counts;
    return fill3(A3);
  }
  Record& background(PB1, int infill_border = 0, int view_surfaces = 0, float surface_max_ratio = 0.f) {          // n_fg = 0, one edit
    this->bg_depth = bg_depth, this->res = res, this->grid_x = grid_x, this->grid_y = grid_y, this->inv_fx = inv_fx;
    this->inv_fy = inv_fy, this->fx = fx, this->fy = fy, this->bounds = bounds, this->zmap = zmap, this->disparity = disparity;
    this->counts = counts, this->workspace = workspace, this->workspace_bytes = workspace_bytes, this->stream = stream;
    this->n_edits = 1, this->views = view, this->has_view = view ? &ONE : nullptr, this->bg_valid = bg_valid;          // (view NULL = no view)
    this->bg_corr = bg_corr, this->bg_counts = bg_counts;
    return settings(infill_border, view_surfaces, surface_max_ratio);
  }
  Record& settings(int infill_border, int view_surfaces = 0, float surface_max_ratio = 0.f) {
    this->infill_border = infill_border, this->view_surfaces = view_surfaces, this->surface_max_ratio = surface_max_ratio;
    return *this;
  }
  // a query: n_pts stands where the call has n_fg (a query has no tables to sum over); n_instances < 0: no table at all; views:
  // the query reserved the view rows whatever the call would bring, which is a view in every edit
  Record& query(int res, int n_pts, int n_edits, int n_objects, int n_instances = -1, int footprints = 0, bool views = false) {
    thread_local std::vector<uint8_t> ones;
    ones.assign(n_edits > 0 ? (size_t)n_edits : 0, 1);
    this->res = res, this->n_fg = n_pts, this->n_edits = n_edits, this->n_objects = n_objects, this->footprints = footprints;
    this->n_instances = n_instances < 0 ? 0 : n_instances != 0 ? n_instances : -1, this->has_view = views ? ones.data() : nullptr;
    return *this;
  }
};

// the rows of the rigid entries (8 doubles) widened to similarity rows: scale 1, no pivot.  The buffer outlives the call (the
// copy to the device is asynchronous), one per calling thread.
const double* rigid_rows(const double* rows8, size_t n) {
  thread_local std::vector<double> wide;
  wide.assign(n * DH_SIMILARITY_ROW, 0.0);
  for (size_t r = 0; r < n; ++r) {
    double* w = wide.data() + r * DH_SIMILARITY_ROW;
    for (int k = 0; k < 8; ++k) w[k] = rows8[r * 8 + k];
    w[8] = w[9] = w[10] = 1.0;
  }
  return wide.data();
}

}  // namespace

// ---- the object entries, oldest first -----------------------------------------------------------------------------------------
// one mask, rigid rows
extern "C" int dh_reproject_edits(const float* depth, const float* bg_depth, const int32_t* fg_pix, int n_fg, int res,
                                  const float* grid_x, const float* grid_y, float inv_fx, float inv_fy, double fx, double fy,
                                  int n_edits, const double* xforms_host, const float* bounds, float* zmap, uint8_t* raw_mask,
                                  uint8_t* clean_mask, float* disparity, uint8_t* vis, int32_t* target_xy, int64_t* corr,
                                  int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  DH_REQUIRE(xforms_host, "null input");
  DH_REQUIRE(n_edits >= 1, "bad sizes");
  const int32_t obj_start[2] = {0, n_fg};
  const int n_objects = 1;
  xforms_host = rigid_rows(xforms_host, (size_t)n_edits);
  return dh_reproject(&Record().fill0(A0));
}

// rigid rows
extern "C" int dh_reproject_object_edits(P0) {
  DH_REQUIRE(xforms_host, "null input");
  DH_REQUIRE(n_edits >= 1, "bad sizes");
  DH_REQUIRE(n_objects >= 1 && n_objects <= MAX_OBJECTS, "1 to 8 objects");
  xforms_host = rigid_rows(xforms_host, (size_t)n_edits * n_objects);
  return dh_reproject(&Record().fill0(A0));
}

// the record that is zero beyond these members
extern "C" int dh_reproject_similarity_edits(P0) { return dh_reproject(&Record().fill0(A0)); }

extern "C" int dh_reproject_footprint_edits(P1) { return dh_reproject(&Record().fill1(A1)); }

extern "C" int dh_reproject_instance_edits(P2) { return dh_reproject(&Record().fill2(A2)); }

extern "C" int dh_reproject_donor_edits(P3) {
  DH_REQUIRE(n_host_objects >= 0, "n_host_objects must lie in 0 .. n_objects");
  return dh_reproject(&Record().fill3(A3));
}

extern "C" int dh_reproject_camera_edits(P4) {
  DH_REQUIRE(n_host_objects >= 0, "n_host_objects must lie in 0 .. n_objects");
  DH_REQUIRE(n_edits >= 1, "bad sizes");
  return dh_reproject(&Record().fill4(A4));
}

extern "C" int dh_reproject_border_edits(P4, int infill_border) {
  DH_REQUIRE(infill_border == 0 || infill_border == 1, "infill_border must be 0 (zero) or 1 (reflect)");
  DH_REQUIRE(n_host_objects >= 0, "n_host_objects must lie in 0 .. n_objects");
  DH_REQUIRE(n_edits >= 1, "bad sizes");
  return dh_reproject(&Record().fill4(A4).settings(infill_border));
}

extern "C" int dh_reproject_surface_edits(P4, int infill_border, int view_surfaces, float surface_max_ratio) {
  DH_REQUIRE(infill_border == 0 || infill_border == 1, "infill_border must be 0 (zero) or 1 (reflect)");
  DH_REQUIRE(n_host_objects >= 0, "n_host_objects must lie in 0 .. n_objects");
  DH_REQUIRE(n_edits >= 1, "bad sizes");
  return dh_reproject(&Record().fill4(A4).settings(infill_border, view_surfaces, surface_max_ratio));
}

// every member of the record (n_bones = 0 means "none" there and was refused here)
extern "C" int dh_reproject_bend_edits(P4, int infill_border, int view_surfaces, float surface_max_ratio, int n_bones,
                                       const float* bone_w) {
  DH_REQUIRE(infill_border == 0 || infill_border == 1, "infill_border must be 0 (zero) or 1 (reflect)");
  DH_REQUIRE(n_host_objects >= 0, "n_host_objects must lie in 0 .. n_objects");
  DH_REQUIRE(n_edits >= 1, "bad sizes");
  DH_REQUIRE(n_bones != 0, "n_bones must lie in 1 .. 4");
  Record a;
  a.fill4(A4).settings(infill_border, view_surfaces, surface_max_ratio);
  a.n_bones = n_bones, a.bone_w = bone_w;
  return dh_reproject(&a);
}

// ---- the entries without a foreground point -----------------------------------------------------------------------------------
extern "C" int dh_reproject_background(PB0) { return dh_reproject(&Record().background(AB0, nullptr, nullptr, nullptr, nullptr)); }

extern "C" int dh_reproject_camera_background(PB1) { return dh_reproject(&Record().background(AB1)); }

extern "C" int dh_reproject_border_background(PB1, int infill_border) { return dh_reproject(&Record().background(AB1, infill_border)); }

extern "C" int dh_reproject_surface_background(PB1, int infill_border, int view_surfaces, float surface_max_ratio) {
  return dh_reproject(&Record().background(AB1, infill_border, view_surfaces, surface_max_ratio));
}

// ---- the workspace queries ----------------------------------------------------------------------------------------------------
extern "C" int dh_reproject_workspace_bytes(int res, int n_fg, int n_edits, size_t* bytes) {
  return dh_reproject_workspace(&Record().query(res, n_fg, n_edits, 1), bytes);
}

extern "C" int dh_reproject_objects_workspace_bytes(int res, int n_fg, int n_edits, int n_objects, size_t* bytes) {
  return dh_reproject_workspace(&Record().query(res, n_fg, n_edits, n_objects), bytes);
}

extern "C" int dh_reproject_footprints_workspace_bytes(int res, int n_fg, int n_edits, int n_objects, int footprints,
                                                       size_t* bytes) {
  return dh_reproject_workspace(&Record().query(res, n_fg, n_edits, n_objects, -1, footprints), bytes);
}

extern "C" int dh_reproject_instances_workspace_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances,
                                                      int footprints, size_t* bytes) {
  return dh_reproject_workspace(&Record().query(res, n_pts, n_edits, n_objects, n_instances > 0 ? n_instances : 0, footprints), bytes);
}

// (a donor changes no size)
extern "C" int dh_reproject_donor_workspace_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances, int footprints,
                                                  size_t* bytes) {
  return dh_reproject_workspace(&Record().query(res, n_pts, n_edits, n_objects, n_instances > 0 ? n_instances : 0, footprints), bytes);
}

extern "C" int dh_reproject_camera_workspace_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances, int footprints,
                                                   size_t* bytes) {
  return dh_reproject_workspace(&Record().query(res, n_pts, n_edits, n_objects, n_instances > 0 ? n_instances : 0, footprints, true), bytes);
}

extern "C" int dh_reproject_surface_ws_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances, int view_surfaces,
                                             size_t* bytes) {
  Record a;
  a.query(res, n_pts, n_edits, n_objects, n_instances > 0 ? n_instances : 0, 0, true).view_surfaces = view_surfaces;
  return dh_reproject_workspace(&a, bytes);
}

extern "C" int dh_reproject_bend_ws_bytes(int res, int n_pts, int n_edits, int n_objects, int n_instances, int view_surfaces,
                                          int footprints, int n_bones, size_t* bytes) {
  DH_REQUIRE(n_bones != 0, "n_bones must lie in 1 .. 4");
  Record a;
  a.query(res, n_pts, n_edits, n_objects, n_instances > 0 ? n_instances : 0, footprints, true).view_surfaces = view_surfaces;
  a.n_bones = n_bones;
  return dh_reproject_workspace(&a, bytes);
}

extern "C" int dh_reproject_background_workspace_bytes(int res, size_t* bytes) {
  DH_REQUIRE(res >= 2 && res <= 32768 && bytes, "bad arguments");
  return dh_reproject_workspace(&Record().query(res, 0, 1, 0), bytes);
}

extern "C" int dh_reproject_surface_background_ws_bytes(int res, int view_surfaces, size_t* bytes) {
  DH_REQUIRE(res >= 2 && res <= 32768 && bytes, "bad arguments");
  Record a;
  a.query(res, 0, 1, 0, -1, 0, true).view_surfaces = view_surfaces;
  return dh_reproject_workspace(&a, bytes);
}
