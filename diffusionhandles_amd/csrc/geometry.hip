// Depth re-projection kernels for gfx950: unproject -> SE(3) -> project -> two-pass
// 64-bit atomic z-buffer -> mask morphology -> ordered compaction of correspondences ->
// harmonic in-fill (single-workgroup f64 CG) -> normalised disparity.
//
// Arithmetic contract (bit-exact integer outputs vs oracle/depth_ref.py, which is pinned
// to the reference depth_transform.py:198-747): float32 where NumPy/torch compute in
// float32, float64 where they compute in float64, no FMA contraction (this TU is built
// with -ffp-contract=off), divisions done in f64 and rounded once (innocuous double
// rounding: 53 >= 2*24+2).
#include "common.h"
#include "compact.h"

#include <vector>

namespace dh {

// ---------------------------------------------------------------------- point geometry
__device__ __forceinline__ void unproject_px(const float* depth, int p, int res, const float* gx, const float* gy,
                                             float ifx, float ify, float& X, float& Y, float& Z) {
  int row = p / res, col = p - row * res;
  float d = depth[p];
  float ax = d * ifx;
  float ay = d * ify;
  X = -(ax * gx[col]);
  Y = -(ay * gy[row]);
  Z = d;
}

__global__ void k_unproject(const float* depth, int res, const float* gx, const float* gy, float ifx, float ify,
                            float* pts) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= res * res) return;
  float X, Y, Z;
  unproject_px(depth, p, res, gx, gy, ifx, ify, X, Y, Z);
  pts[3 * p + 0] = X;
  pts[3 * p + 1] = Y;
  pts[3 * p + 2] = Z;
}

// NumPy's mean over an [N,3] float32 array along axis 0: sequential float32 accumulation in
// row order, then / float32(N).  The additions are inherently serial (bit-exact order); the unprojection is
// not: the whole workgroup stages the next 1024 points into LDS while lanes 0..2 (one coordinate each)
// fold the previous 1024 in order.
//
// Several rigid bodies (dh_reproject_object_edits): object m owns fg_pix[start[m] .. start[m + 1]); the table travels BY VALUE
// in the kernel arguments (the idiom of energy.hip's item table).  Workgroup m folds its own slice, so the M serial chains run
// side by side; entries past the last object hold the total, so no slice index can leave the list.
constexpr int MAX_OBJECTS = 8;
struct ObjTable {
  int start[MAX_OBJECTS + 1];
};
static ObjTable obj_table(int n_objects, const int* obj_start, int n_fg) {
  ObjTable t;
  for (int m = 0; m <= MAX_OBJECTS; ++m) t.start[m] = m < n_objects ? obj_start[m] : n_fg;
  return t;
}

// Copies of an object (dh_reproject_instance_edits): an edit places N INSTANCES, instance n = (mask obj[n], row e * N + n).  The
// point list holds the instances one after the other: instance n owns the positions start[n] .. start[n + 1) (entries past
// the last instance hold n_pts), and position j of it is the source pixel fg_pix[j + off[n]] (off = the start of mask obj[n]
// in fg_pix minus start[n]).  BY VALUE in the kernel arguments, like ObjTable; k_centroid keeps ObjTable (one chain per mask).
// The identity table (N = M, obj[n] = n, off[n] = 0) is the call without copies.
struct InstTable {
  int start[MAX_OBJECTS + 1];
  int off[MAX_OBJECTS];
  int obj[MAX_OBJECTS];
};
static InstTable inst_table(int n_inst, const int* inst_obj, const int* obj_start, int* n_pts_out) {
  InstTable t;
  int at = 0;
  for (int n = 0; n < MAX_OBJECTS; ++n) {
    t.start[n] = at;
    t.off[n] = 0;
    t.obj[n] = 0;
    if (n < n_inst) {
      const int o = inst_obj[n];
      t.off[n] = obj_start[o] - at;
      t.obj[n] = o;
      at += obj_start[o + 1] - obj_start[o];
    }
  }
  t.start[MAX_OBJECTS] = at;
  *n_pts_out = at;
  return t;
}
// the instance of point-list position j: a compare chain against the table's scalars, the offset and the mask by selects along
// it (no indexed read of the by-value table with a per-lane index: that would be a private copy of it)
__device__ __forceinline__ int inst_of(int j, const InstTable& tab, int& off, int& obj) {
  int n = 0;
  off = tab.off[0];
  obj = tab.obj[0];
#pragma unroll
  for (int k = 1; k < MAX_OBJECTS; ++k) {
    const bool in = j >= tab.start[k];
    n += in ? 1 : 0;
    off = in ? tab.off[k] : off;
    obj = in ? tab.obj[k] : obj;
  }
  return n;
}

// Donor objects (dh_reproject_donor_edits): masks n_host .. draw their points from donor_depth, the depth of another image of
// the same resolution and intrinsics.  One workgroup folds one mask, so the select is uniform over the workgroup.  Without a
// donor the entry hands in donor_depth = depth and n_host = the number of masks.
constexpr int CEN_CHUNK = 1024;
__global__ void __launch_bounds__(CEN_CHUNK) k_centroid(const float* depth, const float* donor_depth, int n_host,
                                                         const int* fg_pix, const ObjTable tab, int res,
                                                         const float* gx, const float* gy, float ifx, float ify, float* cen) {
  __shared__ float sv[2][3][CEN_CHUNK];
  const int t = threadIdx.x;
  depth = (int)blockIdx.x >= n_host ? donor_depth : depth;
  const int n = tab.start[blockIdx.x + 1] - tab.start[blockIdx.x];
  fg_pix += tab.start[blockIdx.x];
  cen += 4 * blockIdx.x;
  float acc = 0.f;
  const int nchunks = (n + CEN_CHUNK - 1) / CEN_CHUNK;
  for (int c = 0; c <= nchunks; ++c) {
    if (c < nchunks) {
      const int i = c * CEN_CHUNK + t;
      if (i < n) {
        float X, Y, Z;
        unproject_px(depth, fg_pix[i], res, gx, gy, ifx, ify, X, Y, Z);
        sv[c & 1][0][t] = X; sv[c & 1][1][t] = Y; sv[c & 1][2][t] = Z;
      }
    }
    if (c > 0 && t < 3) {
      const int base = (c - 1) * CEN_CHUNK;
      const int m = n - base < CEN_CHUNK ? n - base : CEN_CHUNK;
      const float* v = sv[(c - 1) & 1][t];
      // the adds are one dependent chain (the order IS the result); what can overlap them is the LDS read of the NEXT
      // batch: two register batches of 16, the loads of one issued before the adds of the other
      int k = 0;
      float u[16], w[16];
      if (m >= 16) {
#pragma unroll
        for (int j = 0; j < 16; ++j) u[j] = v[j];
      }
      for (; k + 32 <= m; k += 32) {
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = v[k + 16 + j];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc = acc + u[j];
        if (k + 48 <= m) {
#pragma unroll
          for (int j = 0; j < 16; ++j) u[j] = v[k + 32 + j];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) acc = acc + w[j];
      }
      if (k + 16 <= m) {          // (u holds v[k .. k+16) here: loaded by the prologue or by the last loop pass)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc = acc + u[j];
        k += 16;
      }
      for (; k < m; ++k) acc = acc + v[k];
    }
    __syncthreads();
  }
  if (t < 3) cen[t] = (float)((double)acc / (double)(float)n);
}

__device__ __forceinline__ unsigned long long sortable_f64(double z) {
  unsigned long long b = (unsigned long long)__double_as_longlong(z);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double unsort_f64(unsigned long long k) {
  unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// One transform row on the device = the row of dh_reproject_similarity_edits (DH_SIMILARITY_ROW doubles, diffhandles_hip.h):
// the 8 doubles of dh_reproject_object_edits, then the scale per camera axis, the pivot and its flag (float32 values widened).
struct Xf {
  double ax, ay, az, c, s, tx, ty, tz;
  double sx, sy, sz, px, py, pz, has_pivot, reserved;
};
static_assert(sizeof(Xf) == DH_SIMILARITY_ROW * sizeof(double), "Xf is the similarity row");

// The arithmetic of one transform row, the ONE statement of it (instances and views): q = fl32(P - c) scaled per camera axis by
// one rounded f32 multiply, f32 cross products and dot, the f64 combination, then (r + (double)c) + t.
__device__ __forceinline__ void xf_apply(const Xf& t, float x, float y, float z, float c0, float c1, float c2, double& X, double& Y,
                                         double& Z) {
  const float q0 = (x - c0) * (float)t.sx, q1 = (y - c1) * (float)t.sy, q2 = (z - c2) * (float)t.sz;
  const float a0 = (float)t.ax, a1 = (float)t.ay, a2 = (float)t.az;
  const float cr0 = a1 * q2 - a2 * q1;
  const float cr1 = a2 * q0 - a0 * q2;
  const float cr2 = a0 * q1 - a1 * q0;
  const float dt = (q0 * a0 + q1 * a1) + q2 * a2;
  const double omc = 1.0 - t.c;
  const double r0 = ((double)q0 * t.c + (double)cr0 * t.s) + (double)(a0 * dt) * omc;
  const double r1 = ((double)q1 * t.c + (double)cr1 * t.s) + (double)(a1 * dt) * omc;
  const double r2 = ((double)q2 * t.c + (double)cr2 * t.s) + (double)(a2 * dt) * omc;
  X = (r0 + (double)c0) + t.tx;
  Y = (r1 + (double)c1) + t.ty;
  Z = (r2 + (double)c2) + t.tz;
}

// Camera moves (dh_reproject_camera_edits; DESIGN.md, "Camera moves"): views = NULL, or one row per edit on the device, the
// INVERSE motion of the edit's camera as a similarity row (scale 1, the pivot always selected); its last double is the edit's
// flag (0 = the edit has no view).  The flag is uniform over a workgroup (blockIdx.y is the edit).
__device__ __forceinline__ bool has_view(const Xf* views, int e) { return views != nullptr && views[e].reserved != 0.0; }

// one thread per (edit, point): points [0,R2) are background pixels, [R2,R2+n_pts) foreground, instance after instance
// (InstTable; without copies an instance is an object).  xf: n_inst rows per edit (edit-major), cen: 4 floats per MASK -- a
// copy does not recompute its mask's centroid.  The instance turns about its row's pivot when the row has
// one (edits of one call may pivot one object differently), else about its mask's centroid; q is scaled per camera axis BEFORE
// the rotation, one rounded f32 multiply per component (s = 1 leaves every bit of q as it was).
// FP (footprint splatting, further down): the foreground points also leave (u, v, Z) -- u, v before the clamp and the
// rounding -- in uvz, 3 doubles per point-list position and edit, for the triangles between them.
// donor_depth, n_host: a point of mask o >= n_host reads the donor's depth (a pointer select beside the inst_of chain).
// views (never with FP): in an edit with a view EVERY point of the list then goes through the view row with the same
// arithmetic, its input the f32 background point or the instance's (X, Y, Z) rounded to f32; such an edit has no clamp: a
// point whose rint(u) or rint(v) (half to even, before any clamp) leaves 0 .. res - 1, or whose Z is not > 0, bids for no
// pixel and leaves pix = -1.  An edit without a view skips all of it behind the uniform flag.
// VS (view surfaces, further down; never with FP): an edit with a view also leaves (u, v, Z) of EVERY point of the list -- after
// the view, before the discard, the clamp and the rounding -- in uvz, 3 doubles per point and edit ([K][P][3]).
// SK (bend edits, dh_reproject_bend_edits; DESIGN.md, "Bend edits"): an instance has n_bones rows per edit (xf is
// [K][n_inst][n_bones]) and point-list position j the weights bone_w[(e * n_pts + j) * n_bones ..], one contiguous load.  The
// point goes to the f64 sum of w_b * xf_apply(row_b) over the bones with w_b != 0, b ascending, the first product opening the
// sum (w = 1 on one bone leaves that bone's bits); all weights 0 = bone 0 with weight 1.  One row is live at a time: the loop
// over the bones is not unrolled and the weight of bone b is a select over scalars, never an indexed private array.
template <bool FP, bool VS = false, bool SK = false>
__global__ void k_points(const float* depth, const float* donor_depth, int n_host, const float* bg_depth, const int* fg_pix,
                         int n_pts, int res,
                         const float* gx, const float* gy, float ifx, float ify, double fx, double fy,
                         const Xf* xf, const float* cen, const InstTable tab, int n_inst, unsigned long long* zbuf,
                         int* pix_out, unsigned long long* key_out, double* uvz, const Xf* views, const float* bone_w,
                         int n_bones) {
  const int R2 = res * res, P = R2 + n_pts;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  if (i >= P) return;
  double X, Y, Z;
  if (i < R2) {
    float x, y, z;
    unproject_px(bg_depth, i, res, gx, gy, ifx, ify, x, y, z);
    X = x; Y = y; Z = z;
  } else {
    // the instance of this point (unused entries of the table hold n_pts: never passed), its source pixel and its mask
    int off, o;
    const int n = inst_of(i - R2, tab, off, o);
    float x, y, z;
    unproject_px(o >= n_host ? donor_depth : depth, fg_pix[i - R2 + off], res, gx, gy, ifx, ify, x, y, z);
    if (!SK) {
      const Xf t = xf[e * n_inst + n];
      // (the centroid is read whether or not the row has a pivot: three selects, no divergent branch around dependent loads)
      const bool piv = t.has_pivot != 0.0;
      const float g0 = cen[4 * o], g1 = cen[4 * o + 1], g2 = cen[4 * o + 2];
      const float c0 = piv ? (float)t.px : g0, c1 = piv ? (float)t.py : g1, c2 = piv ? (float)t.pz : g2;
      xf_apply(t, x, y, z, c0, c1, c2, X, Y, Z);
    } else {
      // the weights of this point: one n_bones-wide load (the entry checks the 16-byte alignment the float4 needs)
      const float* wp = bone_w + ((size_t)e * n_pts + (i - R2)) * n_bones;
      float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
      if (n_bones == 4) {
        const float4 q = *reinterpret_cast<const float4*>(wp);
        w0 = q.x; w1 = q.y; w2 = q.z; w3 = q.w;
      } else if (n_bones == 2) {
        const float2 q = *reinterpret_cast<const float2*>(wp);
        w0 = q.x; w1 = q.y;
      } else if (n_bones == 3) {
        w0 = wp[0]; w1 = wp[1]; w2 = wp[2];
      } else {
        w0 = wp[0];
      }
      if (w0 == 0.f && w1 == 0.f && w2 == 0.f && w3 == 0.f) w0 = 1.f;
      const float g0 = cen[4 * o], g1 = cen[4 * o + 1], g2 = cen[4 * o + 2];
      const Xf* rows = xf + (size_t)(e * n_inst + n) * n_bones;
      bool open = false;
      X = 0.0; Y = 0.0; Z = 0.0;
#pragma unroll 1
      for (int b = 0; b < n_bones; ++b) {
        const float wb = b == 0 ? w0 : b == 1 ? w1 : b == 2 ? w2 : w3;
        if (wb == 0.f) continue;
        const Xf t = rows[b];
        const bool piv = t.has_pivot != 0.0;
        const float c0 = piv ? (float)t.px : g0, c1 = piv ? (float)t.py : g1, c2 = piv ? (float)t.pz : g2;
        double bx, by, bz;
        xf_apply(t, x, y, z, c0, c1, c2, bx, by, bz);
        const double wd = (double)wb;
        bx = wd * bx; by = wd * by; bz = wd * bz;
        X = open ? X + bx : bx;
        Y = open ? Y + by : by;
        Z = open ? Z + bz : bz;
        open = true;
      }
    }
  }
  bool view = false;
  if (!FP) {
    view = has_view(views, e);
    if (view) {
      const Xf v = views[e];
      xf_apply(v, (float)X, (float)Y, (float)Z, (float)v.px, (float)v.py, (float)v.pz, X, Y, Z);
    }
  }
  const double m = (double)(res - 1);
  double u = (fx * (-X)) / Z;
  double v = (fy * (-Y)) / Z;
  u = (u * 0.5 + 0.5) * m;
  v = (v * 0.5 + 0.5) * m;
  if (FP && i >= R2) {
    double* o = uvz + ((size_t)e * n_pts + (i - R2)) * 3;
    o[0] = u; o[1] = v; o[2] = Z;
  }
  if (VS && view) {
    double* o = uvz + ((size_t)e * P + i) * 3;
    o[0] = u; o[1] = v; o[2] = Z;
  }
  const unsigned long long key = sortable_f64(Z);
  if (view) {
    // out of frame: no bid, no row (a NaN fails every comparison).  Inside the frame the clamp below changes nothing.
    const double ru = rint(u), rv = rint(v);
    if (!(ru >= 0.0 && ru <= m && rv >= 0.0 && rv <= m && Z > 0.0)) {
      pix_out[(size_t)e * P + i] = -1;
      key_out[(size_t)e * P + i] = key;
      return;
    }
  }
  u = fmin(fmax(u, 0.0), m);
  v = fmin(fmax(v, 0.0), m);
  const int ui = (int)rint(u), vi = (int)rint(v);
  const int pix = vi * res + ui;
  pix_out[(size_t)e * P + i] = pix;
  key_out[(size_t)e * P + i] = key;
  atomicMin(&zbuf[(size_t)e * R2 + pix], key);
}

// (pix < 0: a point a view put out of frame -- it bid for nothing and owns nothing)
__global__ void k_resolve(int P, int R2, const unsigned long long* zbuf, const int* pix_arr,
                          const unsigned long long* key_arr, int* owner) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  if (i >= P) return;
  int pix = pix_arr[(size_t)e * P + i];
  if (pix < 0) return;
  if (key_arr[(size_t)e * P + i] == zbuf[(size_t)e * R2 + pix]) atomicMin(&owner[(size_t)e * R2 + pix], i);
}

// --------------------------------------------------------------------------- footprints
// Footprint splatting ("Footprint splatting"): the triangles between neighbouring foreground points of ONE object
// bid in the z-buffer of the points.  Every quad of source pixels (x, y) .. (x + 1, y + 1) has two triangles, in the vertex
// order of the reference's depth_to_mesh: half 0 = (v10, v11, v01), half 1 = (v10, v01, v00) with v[row][col]; triangle id =
// 2 * quad + half.  The vertices are the (u, v, Z) k_points<true> left: unclamped, unrounded.  All arithmetic is f64 in the
// written order (this file is built without FMA contraction); fp_setup / fp_bid are the ONE statement of it, shared by the
// thread tier, the wave tier and both z-buffer passes, so a bid recomputed in pass 2 has the bits it had in pass 1.
struct FpTri {
  double u0, v0, z0, u1, v1, z1, u2, v2, z2, area;
  int c0, c1, r0, r1;      // candidate pixel centres, inclusive, inside the image
};
// (the fg_pix positions of the three vertices travel beside the struct as an int3 BY VALUE: as members, the bidder's
// select-by-weight became an indexed load from a private copy of them -- 120 bytes of scratch per lane)

// inverse of fg_pix: source pixel -> position in the point list (the map is -1 elsewhere: memset 0xff before)
__global__ void k_fp_inverse(const int* fg_pix, int n_fg, int* inv) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_fg) inv[fg_pix[j]] = j;
}

// the part of a triangle that no instance changes: F = the fg_pix positions of its three source pixels.  false = a vertex outside
// the masks, or the depth-ratio guard.  BG (view surfaces): a triangle of the background sheet -- F = the source pixels themselves
// (every quad of the image has its two triangles), depth = bg_depth, inv unread.
template <bool BG = false>
__device__ __forceinline__ bool fp_source(int t, int res, const int* inv, const float* depth, float max_ratio, int3& F) {
  const int q = t >> 1, h = t & 1, qy = q / (res - 1), qx = q - qy * (res - 1);
  const int p00 = qy * res + qx, p01 = p00 + 1, p10 = p00 + res, p11 = p10 + 1;
  const int s0 = p10, s1 = h ? p01 : p11, s2 = h ? p00 : p01;
  if (BG) {
    F = make_int3(s0, s1, s2);
  } else {
    F = make_int3(inv[s0], inv[s1], inv[s2]);
    if ((F.x | F.y | F.z) < 0) return false;
  }
  if (max_ratio > 0.f) {          // on the SOURCE depths, f32: a quad across a depth step inside one mask makes no sheet
    const float d0 = depth[s0], d1 = depth[s1], d2 = depth[s2];
    const float zmin = fminf(fminf(d0, d1), d2), zmax = fmaxf(fmaxf(d0, d1), d2);
    if (zmax > zmin * max_ratio) return false;
  }
  return true;
}

// false = the triangle F does not exist for instance n or is dropped (a vertex outside the mask of the instance, Z <= 0,
// non-finite u / v, area <= 0, an empty candidate box).  n is uniform where this is called (a loop counter, a wave's list
// entry): the table is read with scalars.  J holds POINT-LIST positions.
// VS (view surfaces): uvz holds every point of the list, R2 + n_pts per edit, and the pointer handed in is that of the first
// FOREGROUND point of edit 0.  The background is one more "instance", n = MAX_OBJECTS, whose slice is the whole image: the
// point-list positions -R2 .. -1, position j = source pixel - R2, so that the vertex address and the bidder index R2 + j of
// fp_bid are those of the background point itself.
template <bool VS = false>
__device__ __forceinline__ bool fp_setup(const int3 F, int n, int e, int res, int n_pts, const InstTable& tab, const double* uvz,
                                         FpTri& T, int3& J) {
  // fg_pix position -> point-list position of instance n; inside the instance's slice = the pixel is of its mask
  int off, lo, hi;
  if (VS && n == MAX_OBJECTS) {
    off = res * res; lo = -off; hi = 0;
  } else {
    off = tab.off[n]; lo = tab.start[n]; hi = tab.start[n + 1];
  }
  const int j0 = F.x - off, j1 = F.y - off, j2 = F.z - off;
  if (j0 < lo || j0 >= hi || j1 < lo || j1 >= hi || j2 < lo || j2 >= hi) return false;
  const double* base = uvz + (size_t)e * (VS ? res * res + n_pts : n_pts) * 3;
  const double* a = base + (ptrdiff_t)j0 * 3;
  const double* b = base + (ptrdiff_t)j1 * 3;
  const double* c = base + (ptrdiff_t)j2 * 3;
  T.u0 = a[0]; T.v0 = a[1]; T.z0 = a[2];
  T.u1 = b[0]; T.v1 = b[1]; T.z1 = b[2];
  T.u2 = c[0]; T.v2 = c[1]; T.z2 = c[2];
  if (!(T.z0 > 0.0 && T.z1 > 0.0 && T.z2 > 0.0)) return false;
  const double big = 1.7976931348623157e308;
  if (!(fabs(T.u0) <= big && fabs(T.v0) <= big && fabs(T.u1) <= big && fabs(T.v1) <= big && fabs(T.u2) <= big && fabs(T.v2) <= big))
    return false;
  T.area = (T.u0 - T.u1) * (T.v2 - T.v1) - (T.v0 - T.v1) * (T.u2 - T.u1);          // E(v0; v1, v2)
  if (!(T.area > 0.0)) return false;
  // the box is clipped in double: nothing outside the int range is ever converted
  const double lim = (double)(res - 1);
  const double cmin = fmax(ceil(fmin(fmin(T.u0, T.u1), T.u2)), 0.0), cmax = fmin(floor(fmax(fmax(T.u0, T.u1), T.u2)), lim);
  const double rmin = fmax(ceil(fmin(fmin(T.v0, T.v1), T.v2)), 0.0), rmax = fmin(floor(fmax(fmax(T.v0, T.v1), T.v2)), lim);
  if (!(cmin <= cmax && rmin <= rmax)) return false;
  T.c0 = (int)cmin; T.c1 = (int)cmax; T.r0 = (int)rmin; T.r1 = (int)rmax;
  J = make_int3(j0, j1, j2);
  return true;
}

// the bid of triangle T at pixel centre (c, r), if it covers it (inclusive on every edge): pass 1 lowers the z key of the pixel,
// pass 2 lowers the owner among the bids that carry the winning key.  Bidder = the vertex with the largest edge weight, ties
// to the earlier vertex (NumPy's argmax).
__device__ __forceinline__ void fp_bid(const FpTri& T, const int3 J, int c, int r, int pass, int res, int R2, unsigned long long* zbuf, int* owner) {
  const double px = (double)c, py = (double)r;
  const double w0 = (px - T.u1) * (T.v2 - T.v1) - (py - T.v1) * (T.u2 - T.u1);
  const double w1 = (px - T.u2) * (T.v0 - T.v2) - (py - T.v2) * (T.u0 - T.u2);
  const double w2 = (px - T.u0) * (T.v1 - T.v0) - (py - T.v0) * (T.u1 - T.u0);
  if (!(w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0)) return;
  const double b0 = w0 / T.area, b1 = w1 / T.area, b2 = w2 / T.area;
  const double z = (b0 * T.z0 + b1 * T.z1) + b2 * T.z2;
  const unsigned long long key = sortable_f64(z);
  const int pix = r * res + c;
  if (pass == 1) {
    atomicMin(&zbuf[pix], key);
  } else if (zbuf[pix] == key) {
    int j = J.x;
    double wm = w0;
    if (w1 > wm) { j = J.y; wm = w1; }
    if (w2 > wm) j = J.z;
    atomicMin(&owner[pix], R2 + j);
  }
}

// test hook (dh_dbg_footprint_tier): > 0 = the largest candidate box the thread tier walks itself, 0 = the default
constexpr int FP_TIER_DEFAULT = 64;
static int g_fp_tier = 0;
static inline int fp_tier() { return g_fp_tier > 0 ? g_fp_tier : FP_TIER_DEFAULT; }

// thread tier: one thread per (edit, triangle), walking the instances (a uniform loop; without copies exactly one of them has
// the triangle).  A box of more than `tier` candidates goes to the edit's list for the wave tier as (triangle, instance)
// (appended in pass 1; pass 2 replays the list); the result does not depend on `tier`: atomicMin commutes.
// The list holds triangle * MAX_OBJECTS + instance (unsigned: 16 res^2 < 2^32 for every res the CLOSE element admits); an
// instance has at most 2 |mask| triangles, so 2 n_pts entries per edit hold every list (and 2 (res - 1)^2 without copies).
// VS (view surfaces): only the edits with a view draw; after the instances the triangle of the background sheet, instance code
// MAX_OBJECTS.  The list then holds triangle * (MAX_OBJECTS + 1) + code, still 32 bits: 18 res^2 < 2^32 up to res = 15 446,
// and the CLOSE element (res / 50 squared <= MAX_OFFS offsets) stops at res = 3 249.  2 (res - 1)^2 more entries per edit.
template <bool VS>
__device__ __forceinline__ void fp_draw(const int3 F, int n, unsigned t, int e, int pass, int res, int n_pts, const InstTable& tab,
                                        const double* uvz, int tier, unsigned long long* zb, int* ow, unsigned* big_list,
                                        size_t big_stride, int* big_count) {
  FpTri T;
  int3 J;
  if (!fp_setup<VS>(F, n, e, res, n_pts, tab, uvz, T, J)) return;
  const long long cand = (long long)(T.c1 - T.c0 + 1) * (T.r1 - T.r0 + 1);
  if (cand > tier) {
    if (pass == 1) big_list[(size_t)e * big_stride + atomicAdd(&big_count[e], 1)] = t * (MAX_OBJECTS + (VS ? 1 : 0)) + n;
    return;
  }
  for (int r = T.r0; r <= T.r1; ++r)
    for (int c = T.c0; c <= T.c1; ++c) fp_bid(T, J, c, r, pass, res, res * res, zb, ow);
}

template <bool VS>
__global__ void k_fp_tri(int pass, int res, int n_pts, int n_inst, const int* inv, const InstTable tab, const double* uvz,
                         const float* depth, float max_ratio, int tier, unsigned long long* zbuf, int* owner, unsigned* big_list,
                         size_t big_stride, int* big_count, const float* bg_depth, const Xf* views) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  const int nt = 2 * (res - 1) * (res - 1), R2 = res * res;
  if (t >= nt) return;
  if (VS && !has_view(views, e)) return;
  unsigned long long* zb = zbuf + (size_t)e * R2;
  int* ow = owner + (size_t)e * R2;
  int3 F;
  if ((!VS || n_inst > 0) && fp_source(t, res, inv, depth, max_ratio, F))
    for (int n = 0; n < n_inst; ++n) fp_draw<VS>(F, n, (unsigned)t, e, pass, res, n_pts, tab, uvz, tier, zb, ow, big_list, big_stride, big_count);
  if (VS && fp_source<true>(t, res, nullptr, bg_depth, max_ratio, F))
    fp_draw<VS>(F, MAX_OBJECTS, (unsigned)t, e, pass, res, n_pts, tab, uvz, tier, zb, ow, big_list, big_stride, big_count);
}

// wave tier: one 64-lane wave per listed (triangle, instance), the lanes striding over its box
constexpr int FP_WAVE_BLOCKS = 256;
template <bool VS>
__global__ void __launch_bounds__(256) k_fp_wave(int pass, int res, int n_pts, const int* inv, const InstTable tab, const double* uvz,
                                                 const float* depth, float max_ratio, unsigned long long* zbuf, int* owner,
                                                 const unsigned* big_list, size_t big_stride, const int* big_count,
                                                 const float* bg_depth, const Xf* views) {
  const int e = blockIdx.y, lane = threadIdx.x & 63;
  const int R2 = res * res;
  if (VS && !has_view(views, e)) return;
  constexpr unsigned CODES = MAX_OBJECTS + (VS ? 1 : 0);
  const int n = big_count[e];
  unsigned long long* zb = zbuf + (size_t)e * R2;
  int* ow = owner + (size_t)e * R2;
  for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += FP_WAVE_BLOCKS * 4) {
    FpTri T;
    int3 F, J;
    const unsigned ent = __builtin_amdgcn_readfirstlane(big_list[(size_t)e * big_stride + k]);
    const int code = (int)(ent % CODES);
    if (VS && code == MAX_OBJECTS) {
      if (!fp_source<true>((int)(ent / CODES), res, nullptr, bg_depth, max_ratio, F)) continue;
    } else if (!fp_source((int)(ent / CODES), res, inv, depth, max_ratio, F)) {
      continue;
    }
    if (!fp_setup<VS>(F, code, e, res, n_pts, tab, uvz, T, J)) continue;
    const int W = T.c1 - T.c0 + 1, cand = W * (T.r1 - T.r0 + 1);          // (<= res * res: the box lies inside the image)
    for (int i = lane; i < cand; i += 64) {
      const int dr = i / W;
      fp_bid(T, J, T.c0 + (i - dr * W), T.r0 + dr, pass, res, R2, zb, ow);
    }
  }
}

// with footprints a point is visible when it owns at least one pixel (vis zeroed before); keep = foreground-owned target
// pixel inside the cleaned mask; the correspondences are one row per kept TARGET pixel, row-major
__global__ void k_fp_vis(int R2, int n_pts, const int* owner, const uint8_t* raw_mask, uint8_t* vis, const uint8_t* clean,
                         uint8_t* keep) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (p >= R2) return;
  const size_t o = (size_t)e * R2 + p;
  const bool fg = raw_mask[o] != 0;
  if (vis && fg) vis[(size_t)e * n_pts + (owner[o] - R2)] = 1;
  if (keep) keep[o] = (fg && clean[o]) ? 1 : 0;
}

__global__ void k_write_corr_target(int R2, int res, const int* fg_pix, const InstTable tab, const int* owner, const int* keep_idx,
                                    const int* counts, int count_stride, size_t corr_stride, long long* corr, uint8_t* corr_inst) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (r >= counts[e * count_stride]) return;
  const int t = keep_idx[(size_t)e * R2 + r];
  const int j = owner[(size_t)e * R2 + t] - R2;
  int off, o;
  const int n = inst_of(j, tab, off, o);
  const int p = fg_pix[j + off];
  long long* c = corr + ((size_t)e * corr_stride + r) * 4;
  c[0] = p % res;
  c[1] = p / res;
  c[2] = t % res;
  c[3] = t / res;
  if (corr_inst) corr_inst[(size_t)e * corr_stride + r] = (uint8_t)n;
}

// View surfaces, the rows of a call with the setting: an edit with a view takes them per TARGET pixel, row-major.  vis = the
// owner of the pixel is a foreground point (vis of these edits zeroed before); keep_inst = foreground-owned and inside the cleaned
// mask (k_write_corr_target writes the rows); keep_bg = owned by background point o with bg_valid[o] != 0 and outside the cleaned
// mask.  An edit without a view gets no flag: its rows are the point path's.  clean_stride: R2, or 0 for one zero image.
__global__ void k_vs_flags(int R2, int n_pts, const int* owner, const uint8_t* clean, size_t clean_stride, const uint8_t* bg_valid,
                           const Xf* views, uint8_t* vis, uint8_t* keep_inst, uint8_t* keep_bg) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (p >= R2) return;
  const size_t o = (size_t)e * R2 + p;
  uint8_t fi = 0, fb = 0;
  if (has_view(views, e)) {
    const int w = owner[o];                        // (unowned: the initial 0x7f7f7f7f, beyond every point of the list)
    const bool cl = clean[(size_t)e * clean_stride + p] != 0;
    if (w < R2) {
      fb = bg_valid[w] && !cl ? 1 : 0;
    } else if (w < R2 + n_pts) {
      vis[(size_t)e * n_pts + (w - R2)] = 1;
      fi = cl ? 1 : 0;
    }
  }
  if (keep_inst) keep_inst[o] = fi;
  keep_bg[o] = fb;
}

// background row r of edit e: the r-th flagged target pixel t and its owner o, (o % res, o / res, t % res, t / res)
__global__ void k_vs_write_bg(int R2, int res, const int* owner, const int* row_idx, const int* bg_counts, long long* bg_corr) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (r >= bg_counts[e]) return;
  const int t = row_idx[(size_t)e * R2 + r];
  const int o = owner[(size_t)e * R2 + t];
  long long* c = bg_corr + ((size_t)e * R2 + r) * 4;
  c[0] = o % res;
  c[1] = o / res;
  c[2] = t % res;
  c[3] = t / res;
}

// the instance rows of a call with view surfaces: counts[e][0] = the point rows (edits without a view) + the target rows
__global__ void k_vs_add_counts(int K, const int* target_counts, int* counts) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < K) counts[4 * e] += target_counts[e];
}

__device__ __forceinline__ unsigned int sortable_f32(float x) {
  unsigned int b = __float_as_uint(x);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unsort_f32(unsigned int k) {
  unsigned int b = (k >> 31) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(b);
}

// per pixel: depth map, raw fg mask, raw disparity 1/z and its min/max keys.  In an edit with a view a pixel no point reached
// stays out of the min / max (its 1 / inf = 0 would become the minimum); it joins the in-fill set in k_normalize.
constexpr int PIX_PER_THREAD = 16;
__global__ void k_pixels(int R2, const unsigned long long* zbuf, const int* owner, float* zmap, uint8_t* raw_mask,
                         float* disp, unsigned int* minmax, const Xf* views) {
  __shared__ unsigned int smin[4], smax[4];
  int e = blockIdx.y;
  const bool view = has_view(views, e);
  unsigned int kmin = 0xffffffffu, kmax = 0u;
  // PIX_PER_THREAD pixels per thread: 16x fewer workgroups contend on the two min / max words of the edit
#pragma unroll 4
  for (int it = 0; it < PIX_PER_THREAD; ++it) {
    int p = (blockIdx.x * PIX_PER_THREAD + it) * blockDim.x + threadIdx.x;
    if (p >= R2) break;
    size_t o = (size_t)e * R2 + p;
    unsigned long long k = zbuf[o];
    float z = (k == ~0ull) ? __uint_as_float(0x7f800000u) : (float)unsort_f64(k);
    zmap[o] = z;
    int w = owner[o];
    raw_mask[o] = (k != ~0ull && w >= R2) ? 1 : 0;
    float d = (float)(1.0 / (double)z);
    disp[o] = d;
    const unsigned int kd = sortable_f32(d);
    const bool counted = !(view && k == ~0ull);
    kmin = counted && kd < kmin ? kd : kmin;
    kmax = counted && kd > kmax ? kd : kmax;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    unsigned int a = __shfl_xor(kmin, s, 64), b = __shfl_xor(kmax, s, 64);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { smin[wv] = kmin; smax[wv] = kmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
      kmin = smin[i] < kmin ? smin[i] : kmin;
      kmax = smax[i] > kmax ? smax[i] : kmax;
    }
    atomicMin(&minmax[2 * e], kmin);
    atomicMax(&minmax[2 * e + 1], kmax);
  }
}

// (j: a position in the foreground part of the point list, n_pts of them; with copies a source pixel has several)
__global__ void k_fg_vis(int n_pts, int R2, int P, int res, const int* pix_arr, const int* owner, uint8_t* vis,
                         int* target_xy) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  if (j >= n_pts) return;
  int i = R2 + j;
  int pix = pix_arr[(size_t)e * P + i];
  const bool gone = pix < 0;          // out of frame under a view: not visible, target (-1, -1)
  vis[(size_t)e * n_pts + j] = !gone && owner[(size_t)e * R2 + pix] == i ? 1 : 0;
  target_xy[((size_t)e * n_pts + j) * 2 + 0] = gone ? -1 : pix % res;
  target_xy[((size_t)e * n_pts + j) * 2 + 1] = gone ? -1 : pix / res;
}

// binary morphology with an explicit offset list; pixels outside the image are ignored.
__global__ void k_morph(const uint8_t* src, uint8_t* dst, int res, const int2* offs, int n_off, int dilate) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  if (p >= res * res) return;
  const uint8_t* s = src + (size_t)e * res * res;
  int y = p / res, x = p - y * res;
  int acc = dilate ? 0 : 1;
  for (int k = 0; k < n_off; ++k) {
    int yy = y + offs[k].y, xx = x + offs[k].x;
    if (yy < 0 || yy >= res || xx < 0 || xx >= res) continue;
    int v = s[yy * res + xx] ? 1 : 0;
    acc = dilate ? (acc | v) : (acc & v);
    if (acc == dilate) break;          // decided: a set pixel found (dilate) / a clear one (erode); most waves lie in uniform regions
  }
  dst[(size_t)e * res * res + p] = (uint8_t)acc;
}

// The same morphology on BIT rows (res % 32 == 0): a thread owns one 32-pixel word of the output; a tap (dx, dy) is a funnel
// shift of three source words of row y + dy, so the 76 taps of the 10 x 10 closing ellipse cost 76 shifts per 32 pixels instead
// of 76 byte loads per pixel (57 us per pass at K = 8, 512 x 512: 75 GB/s of useful traffic).  Erosion = NOT dilate(NOT x) with
// the same tap list: taps outside the image are ignored either way (clear rows / words of the complemented image).
//   out = inv_out ^ dilate(inv_in ^ src)
__global__ void k_pack_bits(const uint8_t* src, unsigned* dst, int n_words) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  const uint4 a = *reinterpret_cast<const uint4*>(src + (size_t)w * 32), b = *reinterpret_cast<const uint4*>(src + (size_t)w * 32 + 16);
  const unsigned v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned bits = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) bits |= ((v[i] >> (8 * j)) & 0xffu ? 1u : 0u) << (4 * i + j);
  dst[w] = bits;
}
__global__ void k_unpack_bits(const unsigned* src, uint8_t* dst, int n_words) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  const unsigned bits = src[w];
  unsigned v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i] |= ((bits >> (4 * i + j)) & 1u) << (8 * j);
  }
  *reinterpret_cast<uint4*>(dst + (size_t)w * 32) = make_uint4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<uint4*>(dst + (size_t)w * 32 + 16) = make_uint4(v[4], v[5], v[6], v[7]);
}
__global__ void k_morph_bits(const unsigned* src, unsigned* dst, int res, const int2* offs, int n_off, int inv_in, int inv_out) {
  const int wpr = res >> 5;                                  // words per row
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;     // word of this edit's image
  if (idx >= wpr * res) return;
  const unsigned* s = src + (size_t)blockIdx.y * wpr * res;
  const int y = idx / wpr, wx = idx - y * wpr;
  const unsigned flip = inv_in ? 0xffffffffu : 0u;
  unsigned acc = 0;
  for (int k = 0; k < n_off; ++k) {
    const int yy = y + offs[k].y, dx = offs[k].x;            // out(x) |= in(x + dx)
    if (yy < 0 || yy >= res) continue;
    const unsigned* row = s + (size_t)yy * wpr;
    const unsigned c = row[wx] ^ flip;
    const unsigned l = wx > 0 ? row[wx - 1] ^ flip : 0u;     // pixels left of this word (outside the image: clear)
    const unsigned r = wx + 1 < wpr ? row[wx + 1] ^ flip : 0u;
    unsigned v;
    if (dx == 0) v = c;
    else if (dx > 0) v = dx >= 32 ? r : (c >> dx) | (r << (32 - dx));
    else v = dx <= -32 ? l : (c << -dx) | (l >> (32 + dx));
    acc |= v;
  }
  dst[(size_t)blockIdx.y * wpr * res + idx] = inv_out ? ~acc : acc;
}

// (target_views: NULL, or the views of a call with view surfaces -- an edit with a view then keeps no POINT, its rows are taken
// per target pixel)
__global__ void k_keep_flags(int n_pts, int R2, int P, const int* pix_arr, const uint8_t* vis, const uint8_t* clean,
                             uint8_t* keep, const Xf* target_views) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  if (j >= n_pts) return;
  int pix = pix_arr[(size_t)e * P + R2 + j];
  keep[(size_t)e * n_pts + j] =
      (pix >= 0 && vis[(size_t)e * n_pts + j] && clean[(size_t)e * R2 + pix] && !has_view(target_views, e)) ? 1 : 0;
}

// row r of edit e: the r-th kept point-list position, its source pixel through the table, its instance beside it
__global__ void k_write_corr(int n_pts, int res, const int* fg_pix, const InstTable tab, const int* target_xy, const int* keep_idx,
                             const int* counts, int count_stride, size_t corr_stride, long long* corr, uint8_t* corr_inst) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  if (r >= counts[e * count_stride]) return;
  int j = keep_idx[(size_t)e * n_pts + r];
  int off, o;
  const int n = inst_of(j, tab, off, o);
  int p = fg_pix[j + off];
  long long* c = corr + ((size_t)e * corr_stride + r) * 4;
  c[0] = p % res;
  c[1] = p / res;
  c[2] = target_xy[((size_t)e * n_pts + j) * 2 + 0];
  c[3] = target_xy[((size_t)e * n_pts + j) * 2 + 1];
  if (corr_inst) corr_inst[(size_t)e * corr_stride + r] = (uint8_t)n;
}

__global__ void k_count_flags(const uint8_t* f, int n, int* out, int out_stride, int slot) {
  __shared__ int sm[4];
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  int c = (i < n && f[(size_t)e * n + i]) ? 1 : 0;
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += sm[k];
    if (t) atomicAdd(&out[e * out_stride + slot], t);
  }
}

// object removal (dh_reproject_background): flag the pixels that no point of the list reached (the z-buffer still holds its
// initial key); with a zero "clean" image k_normalize turns the flags into the in-fill set
__global__ void k_unowned(int R2, const unsigned long long* zbuf, uint8_t* flag) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= R2) return;
  flag[p] = zbuf[p] == ~0ull ? 1 : 0;
}

// Background rows of an edit with a view: background point i (its source pixel is i) yields a row when bg_valid[i] != 0 (the
// pixel shows the background, not the in-painted depth under a mask), the point owns its target pixel, and that pixel lies
// outside the cleaned foreground mask.  Flagged here, listed in ascending source pixel order by compact(), written below.
// clean_stride: R2, or 0 for one zero image shared by every edit (the background entry).
__global__ void k_bg_row_flags(int R2, int P, const int* pix_arr, const int* owner, const uint8_t* clean, size_t clean_stride,
                               const uint8_t* bg_valid, const Xf* views, uint8_t* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (i >= R2) return;
  uint8_t f = 0;
  if (has_view(views, e) && bg_valid[i]) {
    const int pix = pix_arr[(size_t)e * P + i];
    if (pix >= 0 && owner[(size_t)e * R2 + pix] == i && !clean[(size_t)e * clean_stride + pix]) f = 1;
  }
  flag[(size_t)e * R2 + i] = f;
}

__global__ void k_write_bg_corr(int R2, int P, int res, const int* pix_arr, const int* row_idx, const int* bg_counts,
                                long long* bg_corr) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (r >= bg_counts[e]) return;
  const int i = row_idx[(size_t)e * R2 + r];
  const int t = pix_arr[(size_t)e * P + i];
  long long* c = bg_corr + ((size_t)e * R2 + r) * 4;
  c[0] = i % res;
  c[1] = i / res;
  c[2] = t % res;
  c[3] = t / res;
}

// normalise disparity in place and flag the pixels to in-fill (cleaned xor raw; in an edit with a view also the pixels no point
// reached: zbuf still holds its initial key there)
__global__ void k_normalize(int R2, float* disp, const unsigned int* minmax, const float* bounds,
                            const uint8_t* raw, const uint8_t* clean, uint8_t* inpaint, const unsigned long long* zbuf,
                            const Xf* views) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  int e = blockIdx.y;
  if (p >= R2) return;
  size_t o = (size_t)e * R2 + p;
  const bool unowned = has_view(views, e) && zbuf[o] == ~0ull;
  float lo = bounds ? bounds[0] : unsort_f32(minmax[2 * e]);
  float hi = bounds ? bounds[1] : unsort_f32(minmax[2 * e + 1]);
  float t = disp[o] - lo;
  t = 255.0f * t;
  float den = hi - lo;
  disp[o] = (float)((double)t / (double)den);
  inpaint[o] = ((clean[o] != 0) != (raw[o] != 0)) || unowned ? 1 : 0;
}

// What the in-fill solvers publish in the iteration slot instead of a count when the field is not valid (the host raises):
// -1 = the bounded grid barrier of k_cg_fill_multi ran out; -2 = the iteration cap was reached with the residual still above the
// tolerance (any solver); -3 = the pipelined recurrence broke down (a step length that is not positive and finite).
constexpr int CG_BARRIER_TIMEOUT = -1, CG_NOT_CONVERGED = -2, CG_BREAKDOWN = -3;
// test hook (dh_dbg_cg_max_iter): > 0 = the iteration cap of the in-fill calls that follow, 0 = each call's own
static int g_cg_max_iter = 0;
static inline int cg_cap(int own) { return g_cg_max_iter > 0 ? g_cg_max_iter : own; }

// The image border of the in-fill (infill_border of the border entries): 0 = zero (a neighbour beyond the frame is a known 0: the
// diagonal stays 4), 1 = reflect (the mirror ghost cell x_ghost = x_self: the diagonal of an unknown is the number of its
// neighbours inside the image).  The neighbour tables carry it: a slot holds an unknown's index, CG_NB_NONE (a known or absent
// neighbour) or, under reflect only, CG_NB_FRAME (beyond the frame), and the diagonal is recounted from the slots wherever a
// product reads them -- compares beside loads, no register per unknown.  Under zero no slot holds CG_NB_FRAME, the count is
// exactly 4.0 and every product has the bits it had with the literal.  Every `>= 0` test reads both sentinels as "no unknown".
constexpr int CG_NB_NONE = -1, CG_NB_FRAME = -2;
__device__ __forceinline__ double cg_diag(int u, int d, int l, int r) {
  return (double)(4 - (u == CG_NB_FRAME) - (d == CG_NB_FRAME) - (l == CG_NB_FRAME) - (r == CG_NB_FRAME));
}

// Harmonic in-fill: A x = b with A = D - adjacency(masked), D = 4 I or the in-image degree (above), solved by CG in float64 by ONE
// workgroup per edit (deterministic fixed-tree reductions).  The vectors are indexed by UNKNOWN (compact, coalesced);
// the four neighbour unknowns of every unknown are resolved once through a pixel -> unknown map, so an iteration is
// three streaming passes plus four gathers per unknown.  (Used for holes of more than CG_SLOTS * 1024 pixels; smaller
// ones stay on chip in cg_fill_lds, which visits the unknowns in the same order: identical iterates.)
__global__ void __launch_bounds__(1024) k_cg_fill(int res, float* disp, const uint8_t* inpaint, const int* unk,
                                                  const int* counts, int count_stride, int slot_n, int slot_it,
                                                  double* __restrict__ vx, double* __restrict__ vr, double* __restrict__ vp,
                                                  double* __restrict__ vq, int max_iter,
                                                  double tol2, int* counts_out, const float* rhs_extra, int min_n,
                                                  int* pixmap, int2* nb_ud, size_t nb_ud_stride, int2* nb_lr,
                                                  size_t nb_lr_stride, int border) {
  __shared__ double sm[16];
  const int e = blockIdx.x, R2 = res * res;
  const int off = border ? CG_NB_FRAME : CG_NB_NONE;     // what a slot beyond the frame holds
  const int n = counts[e * count_stride + slot_n];
  if (n <= min_n) return;                                // solved on chip by cg_fill_lds (inside k_cg_fill_multi)
  float* d = disp + (size_t)e * R2;
  const uint8_t* mk = inpaint + (size_t)e * R2;
  const int* U = unk + (size_t)e * R2;
  // (__restrict__: without it every store to q / x / r / p orders the loads of the next element behind it and an iteration
  // is ~20 dependent L2 round trips per pass; with it the loads of an unrolled batch are issued together)
  double* __restrict__ x = vx + (size_t)e * R2;
  double* __restrict__ r = vr + (size_t)e * R2;
  double* __restrict__ p = vp + (size_t)e * R2;
  double* __restrict__ q = vq + (size_t)e * R2;
  int* map = pixmap + (size_t)e * R2;
  int2* __restrict__ nud = nb_ud + (size_t)e * nb_ud_stride;
  int2* __restrict__ nlr = nb_lr + (size_t)e * nb_lr_stride;
  for (int i = threadIdx.x; i < n; i += blockDim.x) map[U[i]] = i;
  __syncthreads();
  double part = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int pix = U[i], y = pix / res, xx = pix - y * res;
    double b = 0.0;
    int2 ud = make_int2(-1, -1), lr = make_int2(-1, -1);
    if (y > 0) { if (!mk[pix - res]) b += (double)d[pix - res]; else ud.x = map[pix - res]; } else ud.x = off;
    if (y < res - 1) { if (!mk[pix + res]) b += (double)d[pix + res]; else ud.y = map[pix + res]; } else ud.y = off;
    if (xx > 0) { if (!mk[pix - 1]) b += (double)d[pix - 1]; else lr.x = map[pix - 1]; } else lr.x = off;
    if (xx < res - 1) { if (!mk[pix + 1]) b += (double)d[pix + 1]; else lr.y = map[pix + 1]; } else lr.y = off;
    if (rhs_extra) b -= (double)rhs_extra[(size_t)e * R2 + pix];
    nud[i] = ud; nlr[i] = lr;
    x[i] = 0.0;
    r[i] = b;
    p[i] = b;
    part += b * b;
  }
  double rs = block_sum(part, sm);
  const double bnorm = rs;
  int it = 0;
  for (; it < max_iter; ++it) {
    if (!(rs > tol2 * bnorm)) break;
    __syncthreads();
    part = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int2 ud = nud[i], lr = nlr[i];
      const double pi = p[i];
      double a = cg_diag(ud.x, ud.y, lr.x, lr.y) * pi;
      if (ud.x >= 0) a -= p[ud.x];
      if (ud.y >= 0) a -= p[ud.y];
      if (lr.x >= 0) a -= p[lr.x];
      if (lr.y >= 0) a -= p[lr.y];
      q[i] = a;
      part += pi * a;
    }
    const double pq = block_sum(part, sm);
    const double alpha = rs / pq;
    part = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      x[i] += alpha * p[i];
      double rr = r[i] - alpha * q[i];
      r[i] = rr;
      part += rr * rr;
    }
    const double rsn = block_sum(part, sm);
    const double beta = rsn / rs;
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = r[i] + beta * p[i];
    rs = rsn;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) d[U[i]] = (float)x[i];
  if (threadIdx.x == 0) counts_out[e * count_stride + slot_it] = it == max_iter && rs > tol2 * bnorm ? CG_NOT_CONVERGED : it;
}


// The iteration of k_cg_fill with the vectors on chip: thread t owns unknowns t, t + 1024, ... (the order that kernel visits
// them in, so every partial sum and therefore every iterate is bit-identical to it), x / r / q live in registers, p in LDS where
// the four neighbours are read through a pixel -> unknown index map.  One iteration is three workgroup barriers and two LDS
// reductions instead of five passes over global memory.  Run by workgroup 0 of a system inside k_cg_fill_multi (round 6: the
// small systems of a batch are solved WHILE the sixteen-workgroup ones run, not in a launch of their own in front of them).
constexpr int CG_SLOTS = 8;      // unknowns per thread: n <= 8192 takes this path
__device__ __forceinline__ void cg_fill_lds(int e, int res, float* disp, const uint8_t* inpaint, const int* unk, const int* counts,
                                            int count_stride, int slot_n, int slot_it, int* pixmap, int max_iter, double tol2,
                                            int* counts_out, const float* rhs_extra, int border) {
  __shared__ double sm[16];
  __shared__ double sp[CG_SLOTS * 1024];
  const int R2 = res * res;
  const int off = border ? CG_NB_FRAME : CG_NB_NONE;
  const int n = counts[e * count_stride + slot_n];
  if (n > CG_SLOTS * 1024) return;
  float* d = disp + (size_t)e * R2;
  const uint8_t* mk = inpaint + (size_t)e * R2;
  const int* U = unk + (size_t)e * R2;
  int* map = pixmap + (size_t)e * R2;
  if (n == 0) {
    if (threadIdx.x == 0) counts_out[e * count_stride + slot_it] = 0;
    return;
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) map[U[i]] = i;
  __syncthreads();
  int nb[CG_SLOTS][4];
  double x[CG_SLOTS], r[CG_SLOTS], q[CG_SLOTS];
  double part = 0.0;
#pragma unroll
  for (int sl = 0; sl < CG_SLOTS; ++sl) {
    const int i = threadIdx.x + sl * 1024;
    x[sl] = 0.0; r[sl] = 0.0; q[sl] = 0.0;
    nb[sl][0] = nb[sl][1] = nb[sl][2] = nb[sl][3] = -1;
    if (i < n) {
      const int pix = U[i], y = pix / res, xx = pix - y * res;
      double b = 0.0;
      if (y > 0) { if (!mk[pix - res]) b += (double)d[pix - res]; else nb[sl][0] = map[pix - res]; } else nb[sl][0] = off;
      if (y < res - 1) { if (!mk[pix + res]) b += (double)d[pix + res]; else nb[sl][1] = map[pix + res]; } else nb[sl][1] = off;
      if (xx > 0) { if (!mk[pix - 1]) b += (double)d[pix - 1]; else nb[sl][2] = map[pix - 1]; } else nb[sl][2] = off;
      if (xx < res - 1) { if (!mk[pix + 1]) b += (double)d[pix + 1]; else nb[sl][3] = map[pix + 1]; } else nb[sl][3] = off;
      if (rhs_extra) b -= (double)rhs_extra[(size_t)e * R2 + pix];
      r[sl] = b;
      sp[i] = b;
      part += b * b;
    }
  }
  double rs = block_sum(part, sm);
  const double bnorm = rs;
  int it = 0;
  for (; it < max_iter; ++it) {
    if (!(rs > tol2 * bnorm)) break;
    __syncthreads();
    part = 0.0;
#pragma unroll
    for (int sl = 0; sl < CG_SLOTS; ++sl) {
      const int i = threadIdx.x + sl * 1024;
      if (i < n) {
        const double pi = sp[i];
        double a = cg_diag(nb[sl][0], nb[sl][1], nb[sl][2], nb[sl][3]) * pi;
        if (nb[sl][0] >= 0) a -= sp[nb[sl][0]];
        if (nb[sl][1] >= 0) a -= sp[nb[sl][1]];
        if (nb[sl][2] >= 0) a -= sp[nb[sl][2]];
        if (nb[sl][3] >= 0) a -= sp[nb[sl][3]];
        q[sl] = a;
        part += pi * a;
      }
    }
    const double pq = block_sum(part, sm);
    const double alpha = rs / pq;
    part = 0.0;
#pragma unroll
    for (int sl = 0; sl < CG_SLOTS; ++sl) {
      const int i = threadIdx.x + sl * 1024;
      if (i < n) {
        x[sl] += alpha * sp[i];
        const double rr = r[sl] - alpha * q[sl];
        r[sl] = rr;
        part += rr * rr;
      }
    }
    const double rsn = block_sum(part, sm);       // its barriers also order the reads of p above before the update below
    const double beta = rsn / rs;
#pragma unroll
    for (int sl = 0; sl < CG_SLOTS; ++sl) {
      const int i = threadIdx.x + sl * 1024;
      if (i < n) sp[i] = r[sl] + beta * sp[i];
    }
    rs = rsn;
  }
#pragma unroll
  for (int sl = 0; sl < CG_SLOTS; ++sl) {
    const int i = threadIdx.x + sl * 1024;
    if (i < n) d[U[i]] = (float)x[sl];
  }
  if (threadIdx.x == 0) counts_out[e * count_stride + slot_it] = it == max_iter && rs > tol2 * bnorm ? CG_NOT_CONVERGED : it;
}

// Holes too large for one CU's LDS: CGM_WGS workgroups per system.  One workgroup is bound by its CU's memory pipe (15 eight-byte
// accesses per unknown and iteration through one L1: 37 us per iteration at 20 000 unknowns, rocprofv3); here every workgroup owns a
// contiguous 1 / CGM_WGS of the unknowns and the workgroups of a system meet at grid-wide SEAMS.  Rounds 3-5 ran the classic
// recurrence with two seams per iteration (one per dot product); round 6 runs the pipelined form with ONE (see the loop).
// A seam = agent-scope release, one arrival counter per system (monotonic: epoch * CGM_WGS), relaxed polling by one lane, one
// agent-scope acquire, __syncthreads (cdna_hip_programming.md Guideline 16); the dot products are per-workgroup partials written
// before the seam and added by everyone in workgroup order afterwards: identical in every workgroup (the convergence test must
// agree: it decides whether the next seam is entered) and deterministic.
constexpr int CG_REPLACE = 50;                 // k_cg_fill_multi: iterations between two residual replacements
constexpr int CGM_WGS = 16, CGM_EPT = 4;       // unknowns per thread <= 4: n <= 16 * 4 * 1024 (r, w, z, s of an unknown: 8 registers; 8 unknowns spilled)
struct CgSync { unsigned arrive; unsigned fail; unsigned pad[30]; double red[2][CGM_WGS]; double red2[2][CGM_WGS]; };
// Forward progress of the seams needs the CGM_WGS workgroups of a system co-resident.  In-order dispatch gives that on an
// otherwise idle chip (a system's workgroups are consecutive blocks, and the chip holds >= 256 of them), but nothing enforces
// it: CU masks, other streams or processes holding the slots.  So every spin is BOUNDED: after CG_SPIN_CAP polls (seconds; a
// normal seam waits microseconds) the poller raises `fail`, every workgroup of the system leaves at its next seam, and the
// iteration count comes back as -1, which the host turns into an error instead of a hung GPU (advisor, round 3).
constexpr unsigned CG_SPIN_CAP = 1u << 21;
typedef __attribute__((address_space(1))) unsigned cg_gu32;
// FENCED: the payload went through plain stores (release: L2 write-back) and is read with plain loads (acquire: stale lines
// dropped).  Otherwise everything shared was stored write-through and is loaded past the caches (agent-scope relaxed atomics on
// 8-byte words, the guide's R1 form): every storing wave drains its stores, one lane counts the arrival -- no fences.
typedef __attribute__((address_space(1))) unsigned long long cg_gu64;
__device__ __forceinline__ void cg_put(double* p, double v) {
  __hip_atomic_store((cg_gu64*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double cg_get(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((cg_gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// returns false when the system has failed (a bounded spin ran out here or in another workgroup): the caller leaves the kernel
template <bool FENCED>
__device__ __forceinline__ bool cg_seam(CgSync* s, unsigned epoch) {
  __shared__ unsigned seam_ok;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (FENCED) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    cg_gu32* ctr = (cg_gu32*)&s->arrive;
    cg_gu32* fail = (cg_gu32*)&s->fail;
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0, ok = 1;
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch * CGM_WGS) {
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 1023u) == 0 && __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ok = 0; break; }
      if (spins > CG_SPIN_CAP) { __hip_atomic_store(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ok = 0; break; }
    }
    if (ok && __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ok = 0;
    if (FENCED) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    seam_ok = ok;
  }
  __syncthreads();
  return seam_ok != 0;
}
__global__ void __launch_bounds__(1024) k_cg_fill_multi(int res, float* disp, const uint8_t* inpaint, const int* unk,
                                                        const int* counts, int count_stride, int slot_n, int slot_it, double* vx,
                                                        double* vr, double* vp0, double* vp1, int max_iter, double tol2,
                                                        int* counts_out, const float* rhs_extra, int min_n, int* pixmap,
                                                        int2* nb_ud, size_t nb_ud_stride, int2* nb_lr, size_t nb_lr_stride,
                                                        CgSync* sync, int border) {
  __shared__ double sm[16];
  const int e = blockIdx.y, wg = blockIdx.x, R2 = res * res;
  const int n = counts[e * count_stride + slot_n];
  if (n <= min_n) {                                                 // small enough for one CU's LDS: workgroup 0 solves it on chip
    if (wg == 0 && min_n > 0)
      cg_fill_lds(e, res, disp, inpaint, unk, counts, count_stride, slot_n, slot_it, pixmap, max_iter, tol2, counts_out, rhs_extra,
                  border);
    return;
  }
  if (n > CGM_WGS * CGM_EPT * 1024) return;                        // (uniform over the system's workgroups)
  CgSync* sy = sync + e;
  float* d = disp + (size_t)e * R2;
  const uint8_t* mk = inpaint + (size_t)e * R2;
  const int* U = unk + (size_t)e * R2;
  double* x = vx + (size_t)e * R2;
  double* r = vr + (size_t)e * R2;
  double* P[2] = {vp0 + (size_t)e * R2, vp1 + (size_t)e * R2};
  int* map = pixmap + (size_t)e * R2;
  int2* nud = nb_ud + (size_t)e * nb_ud_stride;
  int2* nlr = nb_lr + (size_t)e * nb_lr_stride;
  const int per = (n + CGM_WGS - 1) / CGM_WGS, i0 = wg * per, i1 = i0 + per < n ? i0 + per : n;
  unsigned epoch = 0;
  // The iteration count is published with atomicMin over a slot that workgroup 0 arms here, BEFORE its first seam: a workgroup
  // whose bounded spin runs out on the LAST seam (the others have read fail == 0, pass it and write their slices) still leaves
  // -1 in the slot whatever the order of the two updates, so the host never sees a count >= 0 beside a partly written
  // disparity.  (A failure before workgroup 0 even started is seen by workgroup 0 at its first seam: the flag is sticky.)
  if (wg == 0 && threadIdx.x == 0) atomicExch(&counts_out[e * count_stride + slot_it], 0x7fffffff);
  for (int i = i0 + (int)threadIdx.x; i < i1; i += 1024) map[U[i]] = i;
  bool alive = cg_seam<true>(sy, ++epoch);                           // every workgroup's part of the pixel -> unknown map (plain stores / loads)
  if (!alive) { if (threadIdx.x == 0) atomicMin(&counts_out[e * count_stride + slot_it], -1); return; }
  // PIPELINED conjugate gradients (Ghysels & Vanroose; round 6): with w = A r carried by recurrence, the two dot products of an
  // iteration -- gamma = (r, r), delta = (w, r) -- are taken from the SAME state and the matrix product of the iteration, q = A w,
  // needs nothing from them, so an iteration has ONE grid-wide seam (the partial sums and the new w are published before it)
  // instead of two; the classic recurrence above pays a seam per dot product, 92 x 2 x 6.5 us on the largest hole of the K = 8
  // benchmark call.  Per iteration:   beta = gamma / gamma', alpha = gamma / (delta - beta gamma / alpha')   (first: 0, gamma / delta)
  //     z = q + beta z,  s = w + beta s,  p = r + beta p,   x += alpha p,  r -= alpha s,  w -= alpha z.
  // r, w, z, s of a thread's unknowns live in registers; x and p are private global arrays (p takes over the array the
  // right-hand side was exchanged through); only w is shared, double-buffered (neighbours read the old one while the new one is
  // written).  Same fixed point as cg_fill_lds / k_cg_fill (the iterates differ in rounding: f64, relative residual 1e-12).
  // The recurrences alone drift apart on the larger holes; every CG_REPLACE-th iteration ties them back to x and p (in the loop).
  double* pv = r;                                // b is exchanged through this array during the set-up; afterwards it holds p
  double rl[CGM_EPT], wl[CGM_EPT], zl[CGM_EPT], sl[CGM_EPT];
  double part = 0.0;
#pragma unroll
  for (int k = 0; k < CGM_EPT; ++k) {
    const unsigned i = (unsigned)i0 + threadIdx.x + k * 1024u;
    rl[k] = 0.0; wl[k] = 0.0; zl[k] = 0.0; sl[k] = 0.0;
    if (i < (unsigned)i1) {
      const int pix = U[i], y = pix / res, xx = pix - y * res;
      const int off = border ? CG_NB_FRAME : CG_NB_NONE;
      double b = 0.0;
      int2 ud = make_int2(-1, -1), lr = make_int2(-1, -1);
      if (y > 0) { if (!mk[pix - res]) b += (double)d[pix - res]; else ud.x = map[pix - res]; } else ud.x = off;
      if (y < res - 1) { if (!mk[pix + res]) b += (double)d[pix + res]; else ud.y = map[pix + res]; } else ud.y = off;
      if (xx > 0) { if (!mk[pix - 1]) b += (double)d[pix - 1]; else lr.x = map[pix - 1]; } else lr.x = off;
      if (xx < res - 1) { if (!mk[pix + 1]) b += (double)d[pix + 1]; else lr.y = map[pix + 1]; } else lr.y = off;
      if (rhs_extra) b -= (double)rhs_extra[(size_t)e * R2 + pix];
      nud[i] = ud; nlr[i] = lr;                  // (read back by this thread only)
      x[i] = 0.0;
      cg_put(r + i, b);
      rl[k] = b;
      part += b * b;
    }
  }
  // partials of this workgroup -> seam -> sums in workgroup order (identical in every workgroup: the convergence test must agree)
  auto all_sum2 = [&](double v0, double v1, int slot, double& t0, double& t1) {
    v0 = block_sum(v0, sm);
    v1 = block_sum(v1, sm);
    if (threadIdx.x == 0) { cg_put(&sy->red[slot][wg], v0); cg_put(&sy->red2[slot][wg], v1); }
    if (!cg_seam<false>(sy, ++epoch)) alive = false;
    t0 = 0.0; t1 = 0.0;
    for (int k = 0; k < CGM_WGS; ++k) { t0 += cg_get(&sy->red[slot][k]); t1 += cg_get(&sy->red2[slot][k]); }
  };
  double bnorm, unused;
  all_sum2(part, 0.0, 0, bnorm, unused);        // (the seam also makes every workgroup's b visible)
  if (!alive) { if (threadIdx.x == 0) atomicMin(&counts_out[e * count_stride + slot_it], -1); return; }
#pragma unroll
  for (int k = 0; k < CGM_EPT; ++k) {           // w = A r (r = b: x starts at zero)
    const unsigned i = (unsigned)i0 + threadIdx.x + k * 1024u;
    if (i < (unsigned)i1) {
      const int2 ud = nud[i], lr = nlr[i];
      double a = cg_diag(ud.x, ud.y, lr.x, lr.y) * rl[k];
      if (ud.x >= 0) a -= cg_get(r + ud.x);
      if (ud.y >= 0) a -= cg_get(r + ud.y);
      if (lr.x >= 0) a -= cg_get(r + lr.x);
      if (lr.y >= 0) a -= cg_get(r + lr.y);
      wl[k] = a;
      cg_put(P[0] + i, a);
    }
  }
  // the right-hand side of unknown i again (the set-up's sum, in its order), for the residual replacement
  auto rhs_of = [&](unsigned i) {
    const int pix = U[i], y = pix / res, xx = pix - y * res;
    double b = 0.0;
    if (y > 0 && !mk[pix - res]) b += (double)d[pix - res];
    if (y < res - 1 && !mk[pix + res]) b += (double)d[pix + res];
    if (xx > 0 && !mk[pix - 1]) b += (double)d[pix - 1];
    if (xx < res - 1 && !mk[pix + 1]) b += (double)d[pix + 1];
    if (rhs_extra) b -= (double)rhs_extra[(size_t)e * R2 + pix];
    return b;
  };
  // A v at unknown i: the own value from a register, the neighbours' read past the caches from the array v was published in
  auto lap_at = [&](const double* v, double own, int2 ud, int2 lr) {
    double a = cg_diag(ud.x, ud.y, lr.x, lr.y) * own;
    if (ud.x >= 0) a -= cg_get(v + ud.x);
    if (ud.y >= 0) a -= cg_get(v + ud.y);
    if (lr.x >= 0) a -= cg_get(v + lr.x);
    if (lr.y >= 0) a -= cg_get(v + lr.y);
    return a;
  };
  // an index the compiler cannot see through: the addresses of the loop's accesses are formed where they are used (a shift and an
  // add per access, beside loads that go past the caches) instead of being hoisted out of the loop, where four unknowns x seven
  // arrays of 64-bit addresses, kept alive across the replacement, spilled to scratch (116 .. 148 bytes per lane; now none)
  auto cold_index = [](unsigned i) { asm volatile("" : "+v"(i)); return i; };
  double gamma_old = 1.0, alpha_old = 1.0;
  int cur = 0, it = 0, code = 0;
  for (;; ++it) {
    double pg = 0.0, pd = 0.0;
#pragma unroll
    for (int k = 0; k < CGM_EPT; ++k) { pg += rl[k] * rl[k]; pd += wl[k] * rl[k]; }
    double gamma, delta;
    all_sum2(pg, pd, (it + 1) & 1, gamma, delta);     // (slots alternate: a workgroup still adding one cannot be overtaken by the next write to it)
    if (!alive) break;
    if (!(gamma > tol2 * bnorm)) break;
    if (it >= max_iter) { code = CG_NOT_CONVERGED; break; }      // (gamma is the residual of iterate max_iter itself: one seam more than the cap)
    const double beta = it ? gamma / gamma_old : 0.0;
    const double alpha = it ? gamma / (delta - beta * gamma / alpha_old) : gamma / delta;
    // BREAKDOWN GUARD.  A is positive definite, so in exact arithmetic the denominator is (p, A p) > 0; a step that is not
    // positive and finite means the recurred delta has drifted off it (or carries a NaN).  Nothing of it reaches x: the system
    // leaves with CG_BREAKDOWN and no disparity written (gamma, delta are identical in every workgroup: they all leave here).
    if (!(alpha > 0.0 && alpha <= 1.7976931348623157e308)) { code = CG_BREAKDOWN; break; }
    // RESIDUAL REPLACEMENT (Cools, Yetkin, Agullo, Giraud & Vanroose 2018, without their automatic criterion: a fixed period).
    // r, w, s, z are carried by recurrence, each with its own rounding error, and nothing ties them back to x and p; from
    // ~40 000 unknowns on (some 700 iterations of the classic recurrence) the drift of w - A r and s - A p makes the recurred
    // delta useless: denominators turn negative and the solve takes 1.5 .. 20 x the classic iteration count or runs into the
    // cap, at the same final accuracy.  So every CG_REPLACE-th iteration ends with   r = b - A x,  s = A p,  then  w = A r,
    // z = A s   from the true x and p.  x and p are private otherwise; on these iterations they are also published.
    const bool replace = (it + 1) % CG_REPLACE == 0;
    const double* wo = P[cur];
    double* wn = P[cur ^ 1];
#pragma unroll
    for (int k = 0; k < CGM_EPT; ++k) {
      const unsigned i = cold_index((unsigned)i0 + threadIdx.x + k * 1024u);
      if (i < (unsigned)i1) {
        const int2 ud = nud[i], lr = nlr[i];
        const double q = lap_at(wo, wl[k], ud, lr);
        zl[k] = q + beta * zl[k];
        sl[k] = wl[k] + beta * sl[k];
        const double pk = it ? rl[k] + beta * pv[i] : rl[k];
        const double xk = x[i] + alpha * pk;
        rl[k] -= alpha * sl[k];
        wl[k] -= alpha * zl[k];
        pv[i] = pk;
        x[i] = xk;
        if (replace) {                           // (after the plain stores: this thread's own plain loads keep seeing what they always saw)
          cg_put(pv + i, pk);
          cg_put(x + i, xk);
          sl[k] = pk; zl[k] = xk;                // (p and x of this unknown, carried to the products below)
        } else {
          cg_put(wn + i, wl[k]);
        }
      }
    }
    if (replace) {
      // three seams more than a plain iteration: (1) x and p of every workgroup visible, and nobody still reads wo;
      // r = b - A x goes through wo, s = A p through wn; (2) both visible: w = A r, z = A s; (3) nobody still reads wn,
      // which then takes the new w as on every other iteration.
      if (!cg_seam<false>(sy, ++epoch)) { alive = false; break; }
#pragma unroll
      for (int k = 0; k < CGM_EPT; ++k) {
        const unsigned i = cold_index((unsigned)i0 + threadIdx.x + k * 1024u);
        if (i < (unsigned)i1) {
          const int2 ud = nud[i], lr = nlr[i];
          rl[k] = rhs_of(i) - lap_at(x, zl[k], ud, lr);
          sl[k] = lap_at(pv, sl[k], ud, lr);
          cg_put(P[cur] + i, rl[k]);
          cg_put(wn + i, sl[k]);
        }
      }
      if (!cg_seam<false>(sy, ++epoch)) { alive = false; break; }
#pragma unroll
      for (int k = 0; k < CGM_EPT; ++k) {
        const unsigned i = cold_index((unsigned)i0 + threadIdx.x + k * 1024u);
        if (i < (unsigned)i1) {
          const int2 ud = nud[i], lr = nlr[i];
          wl[k] = lap_at(wo, rl[k], ud, lr);
          zl[k] = lap_at(wn, sl[k], ud, lr);
        }
      }
      if (!cg_seam<false>(sy, ++epoch)) { alive = false; break; }
#pragma unroll
      for (int k = 0; k < CGM_EPT; ++k) {
        const unsigned i = cold_index((unsigned)i0 + threadIdx.x + k * 1024u);
        if (i < (unsigned)i1) cg_put(wn + i, wl[k]);
      }
    }
    gamma_old = gamma; alpha_old = alpha;
    cur ^= 1;
  }
  if (!alive) { if (threadIdx.x == 0) atomicMin(&counts_out[e * count_stride + slot_it], CG_BARRIER_TIMEOUT); return; }
  // not converged / broken down: the code instead of a count, and the disparity stays unwritten (all workgroups agree on it)
  if (code == 0)
    for (int i = i0 + (int)threadIdx.x; i < i1; i += 1024) d[U[i]] = (float)x[i];
  if (threadIdx.x == 0 && wg == 0) atomicMin(&counts_out[e * count_stride + slot_it], code ? code : it);      // (a -1 of another workgroup stays, unless this is a code below it)
}

// cross-element binary dilation (scipy.ndimage.binary_dilation default structure, border 0)
__global__ void k_dilate_cross(const uint8_t* src, uint8_t* dst, int res) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= res * res) return;
  int y = p / res, x = p - y * res;
  int v = src[p];
  if (y > 0) v |= src[p - res];
  if (y < res - 1) v |= src[p + res];
  if (x > 0) v |= src[p - 1];
  if (x < res - 1) v |= src[p + 1];
  dst[p] = v ? 1 : 0;
}
// 5-point Laplacian, f64 sum rounded to f32.  border 0: zero padding (scipy.ndimage.convolve(mode='constant')); 1: replicate
// padding (mode='nearest'): a neighbour beyond the frame is the pixel itself, so the centre weight is the in-image degree
__global__ void k_laplacian(const float* img, float* out, int res, int border) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= res * res) return;
  int y = p / res, x = p - y * res;
  const int deg = border ? (y > 0) + (y < res - 1) + (x > 0) + (x < res - 1) : 4;
  double a = -(double)deg * (double)img[p];
  if (y > 0) a += (double)img[p - res];
  if (y < res - 1) a += (double)img[p + res];
  if (x > 0) a += (double)img[p - 1];
  if (x < res - 1) a += (double)img[p + 1];
  out[p] = (float)a;
}

// OpenCV's classic MORPH_ELLIPSE rows, as (dx, dy) offsets from the anchor
static int ellipse_offsets(int k, int2* out) {
  int n = 0;
  if (k <= 1) {
    out[n++] = make_int2(0, 0);
    return n;
  }
  const int r = k / 2, c = k / 2;
  const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
  for (int i = 0; i < k; ++i) {
    int dy = i - r;
    if (abs(dy) > r) continue;
    int dx = (int)nearbyint(c * sqrt((r * r - dy * dy) * inv_r2));
    int j1 = c - dx > 0 ? c - dx : 0, j2 = c + dx + 1 < k ? c + dx + 1 : k;
    for (int j = j1; j < j2; ++j) out[n++] = make_int2(j - c, i - r);
  }
  return n;
}

constexpr int MAX_OFFS = 4096;

}  // namespace dh
// test hook (host only, no device call): the (dx, dy) offsets of the k x k elliptical structuring element the mask
// clean-up uses, so the CPU suite can pin them to OpenCV's published tables
extern "C" int dh_dbg_ellipse_offsets(int k, int32_t* xy, int cap, int* n_out) {
  DH_REQUIRE(k >= 1 && (long)k * k <= dh::MAX_OFFS && xy && n_out && cap >= k * k, "bad arguments");
  static int2 tmp[dh::MAX_OFFS];
  const int n = dh::ellipse_offsets(k, tmp);
  for (int i = 0; i < n; ++i) { xy[2 * i] = tmp[i].x; xy[2 * i + 1] = tmp[i].y; }
  *n_out = n;
  return DH_OK;
}
// test hooks (host only): the dispatch limits of the in-fill solvers {largest n solved on chip, largest n of the multi-workgroup
// kernel, its workgroups per system}, and an iteration cap for the in-fill calls that follow (0 restores each call's own)
extern "C" int dh_dbg_cg_limits(int* out3) {
  DH_REQUIRE(out3, "bad arguments");
  out3[0] = dh::CG_SLOTS * 1024; out3[1] = dh::CGM_WGS * dh::CGM_EPT * 1024; out3[2] = dh::CGM_WGS;
  return DH_OK;
}
extern "C" int dh_dbg_cg_max_iter(int cap) {
  DH_REQUIRE(cap >= 0, "bad arguments");
  dh::g_cg_max_iter = cap;
  return DH_OK;
}
// test hook (host only): the largest candidate box of a footprint triangle that the thread tier draws itself in the calls that
// follow (larger boxes go to the wave tier); 0 restores the default
extern "C" int dh_dbg_footprint_tier(int tier) {
  DH_REQUIRE(tier >= 0, "bad arguments");
  dh::g_fp_tier = tier;
  return DH_OK;
}
namespace dh {

struct ReprojectWs {
  Xf* xf;
  float* cen;
  unsigned long long* zbuf;
  int* owner;
  int* pix;
  unsigned long long* key;
  unsigned int* minmax;
  uint8_t* tmp_a;
  uint8_t* tmp_b;
  uint8_t* keep;
  uint8_t* inpaint;
  int* keep_idx;
  int* unk;
  int* block_counts;
  int2* offs_close;
  int2* offs_open;
  double *vx, *vr, *vp, *vq;
  CgSync* cgsync;
  // footprints only (nothing is taken without them: the workspace of the other entries is what it was)
  double* uvz;
  int* inv;
  unsigned* big_list;
  int* big_count;
  size_t big_stride;
  // camera moves only (a call in which no edit has a view takes nothing: its workspace is what it was)
  Xf* views;
  // view surfaces only (a view edit with the setting; they share the footprints' members, never taken together): uvz then
  // holds every point of the list, inv only with foreground points, and the list has the background's slots too
};

// n_fg: the foreground points of the point list (with copies n_pts, the sum over the instances); M: masks; N: transform rows
// per edit (instances; 0 = M, the call without copies, whose carving -- and so every workspace query that existed before the
// copies -- is what it was: the wave tier's list then has a slot per triangle of the grid, else 2 n_pts per edit)
// (B: rows per instance, the bones of a bend edit; 1 = every carving that existed before them)
struct CarveSpec {
  int res, n_fg, K, M, N, B;
  bool footprints, camera, surfaces;
};

// What a record carves, for the call and for the query alike.  n_pts and any_view are the two facts they learn differently (the
// call from its checked tables and view rows, the query from what the record says).  Without a foreground point the view lives
// in the one transform row the carving holds, so nothing is taken for it.  View surfaces act only where there is a view.
static CarveSpec carve_spec(const dh_reproject_args& a, int n_pts, bool any_view) {
  const bool surfaces = any_view && a.view_surfaces != 0;
  if (a.n_fg == 0) return {a.res, 0, a.n_edits, a.n_objects > 0 ? a.n_objects : 1, 0, 1, false, false, surfaces};
  return {a.res, n_pts, a.n_edits, a.n_objects, a.inst_obj || a.n_instances ? a.n_instances : 0, a.n_bones > 1 ? a.n_bones : 1,
          a.footprints != 0, any_view, surfaces};
}

static bool carve(Arena& a, const CarveSpec& s, ReprojectWs& w) {
  const int res = s.res, n_fg = s.n_fg, K = s.K, M = s.M, N = s.N, B = s.B;
  const bool footprints = s.footprints, camera = s.camera, surfaces = s.surfaces;
  const size_t R2 = (size_t)res * res, P = R2 + n_fg;
  w.xf = a.take<Xf>((size_t)K * (N > 0 ? N : M) * B);
  w.cen = a.take<float>(4 * M);
  w.zbuf = a.take<unsigned long long>(K * R2);
  w.owner = a.take<int>(K * R2);
  w.pix = a.take<int>(K * P);
  w.key = a.take<unsigned long long>(K * P);
  w.minmax = a.take<unsigned int>(2 * K);
  w.tmp_a = a.take<uint8_t>(K * R2);
  w.tmp_b = a.take<uint8_t>(K * R2);
  w.keep = a.take<uint8_t>((size_t)K * (n_fg > 0 ? n_fg : 1));
  w.inpaint = a.take<uint8_t>(K * R2);
  w.keep_idx = a.take<int>((size_t)K * (n_fg > 0 ? n_fg : 1));
  w.unk = a.take<int>(K * R2);
  w.block_counts = a.take<int>((size_t)K * (cdiv((int)P, CP_TILE) + 1));
  w.offs_close = a.take<int2>(MAX_OFFS);
  w.offs_open = a.take<int2>(MAX_OFFS);
  w.vx = a.take<double>(K * R2);
  w.vr = a.take<double>(K * R2);
  w.vp = a.take<double>(K * R2);
  w.vq = a.take<double>(K * R2);
  w.cgsync = a.take<CgSync>(K);
  w.uvz = nullptr; w.inv = nullptr; w.big_list = nullptr; w.big_count = nullptr; w.big_stride = 0;
  if (footprints) {
    w.uvz = a.take<double>((size_t)K * n_fg * 3);
    w.inv = a.take<int>(R2);
    w.big_stride = N > 0 ? (size_t)2 * n_fg : (size_t)2 * (res - 1) * (res - 1);
    w.big_list = a.take<unsigned>((size_t)K * w.big_stride);
    w.big_count = a.take<int>(K);
  }
  w.views = camera ? a.take<Xf>(K) : nullptr;
  if (surfaces) {
    w.uvz = a.take<double>((size_t)K * P * 3);
    w.inv = n_fg > 0 ? a.take<int>(R2) : nullptr;
    w.big_stride = (size_t)2 * n_fg + (size_t)2 * (res - 1) * (res - 1);
    w.big_list = a.take<unsigned>((size_t)K * w.big_stride);
    w.big_count = a.take<int>(K);
  }
  return a.ok();
}

}  // namespace dh

using namespace dh;

extern "C" int dh_fg_pixel_list(const uint8_t* fg_mask, int res, int32_t* fg_pix, int32_t* n_fg_dev, void* workspace,
                                size_t workspace_bytes, void* stream) {
  DH_REQUIRE(fg_mask && fg_pix && n_fg_dev && workspace, "null pointer");
  int n = res * res;
  DH_REQUIRE(workspace_bytes >= (size_t)(cdiv(n, CP_TILE) + 1) * sizeof(int), "workspace too small");
  compact(fg_mask, n, 1, 0, fg_pix, 0, n_fg_dev, 1, (int*)workspace, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_unproject(const float* depth, int res, const float* grid_x, const float* grid_y, float inv_fx,
                            float inv_fy, float* points, void* stream) {
  DH_REQUIRE(depth && grid_x && grid_y && points && res >= 2, "bad arguments");
  hipLaunchKernelGGL(k_unproject, dim3(cdiv(res * res, 256)), dim3(256), 0, (hipStream_t)stream, depth, res, grid_x,
                     grid_y, inv_fx, inv_fy, points);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_masked_centroid(const float* depth, const int32_t* fg_pix, int n_fg, int res, const float* grid_x,
                                  const float* grid_y, float inv_fx, float inv_fy, float* centroid, void* stream) {
  DH_REQUIRE(depth && fg_pix && centroid && n_fg > 0, "bad arguments");
  const int one[2] = {0, n_fg};
  hipLaunchKernelGGL(k_centroid, dim3(1), dim3(CEN_CHUNK), 0, (hipStream_t)stream, depth, depth, 1, fg_pix, obj_table(1, one, n_fg), res,
                     grid_x, grid_y, inv_fx, inv_fy, centroid);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// Camera moves: the view rows of a call as the device takes them -- the caller's rows with has_view[e] in the last double
// (a row without a view is all zero).  NULL when no edit has a view: that call is the call of the entries without the
// arguments, launch for launch.  ok = false: a view row is malformed (checked as the transform rows are).  The buffer
// outlives the call (the copy to the device is asynchronous), one per calling thread.
// One similarity row, members 8 .. 14: a scale that is not positive and finite would collapse or mirror the object or spread NaN
// over the z-buffer; a pivot is checked whether or not the row's flag selects it.  why: the refusal of a transform row.
static bool row_ok(const double* row, const char** why) {
  const double big = 3.4028234663852886e38;
  *why = "transform row: the scale must be positive and finite";
  for (int k = 8; k < 11; ++k)
    if (!((float)row[k] > 0.0f && row[k] <= big)) return false;
  *why = "transform row: the pivot must be finite";
  for (int k = 11; k < 14; ++k)
    if (!(row[k] >= -big && row[k] <= big)) return false;
  *why = "transform row: the has-pivot flag must be 0 or 1";
  return row[14] == 0.0 || row[14] == 1.0;
}

static const double* view_rows(const double* views, const uint8_t* has_view, int K, bool* ok) {
  thread_local std::vector<double> rows;
  *ok = true;
  bool any = false;
  if (views && has_view)
    for (int e = 0; e < K; ++e) any = any || has_view[e] != 0;
  if (!any) return nullptr;
  rows.assign((size_t)K * DH_SIMILARITY_ROW, 0.0);
  for (int e = 0; e < K; ++e) {
    if (!has_view[e]) continue;
    const double* row = views + (size_t)e * DH_SIMILARITY_ROW;
    double* w = rows.data() + (size_t)e * DH_SIMILARITY_ROW;
    const double big = 3.4028234663852886e38;
    const char* why;
    for (int k = 0; k < 8; ++k) *ok = *ok && row[k] >= -big && row[k] <= big;          // axis, cos, sin, translation: finite
    *ok = *ok && row_ok(row, &why);
    for (int k = 0; k < DH_SIMILARITY_ROW - 1; ++k) w[k] = row[k];
    w[DH_SIMILARITY_ROW - 1] = 1.0;
  }
  return rows.data();
}

// The one launch of k_points<FP, VS, SK>: footprints, view surfaces (never with footprints: refused before any launch, so six
// instances exist) and bones; `args` is the kernel's argument list after the stream.
template <class... A>
static void launch_points(bool fp, bool vs, bool sk, dim3 grid, hipStream_t st, A... args) {
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, args...); };
  if (vs) sk ? go(k_points<false, true, true>) : go(k_points<false, true, false>);
  else if (fp) sk ? go(k_points<true, false, true>) : go(k_points<true, false, false>);
  else sk ? go(k_points<false, false, true>) : go(k_points<false, false, false>);
}

// The triangle kernels of one z-buffer pass over K edits: thread tier, then wave tier (the list is built in pass 1).  VS: view
// surfaces (bg_depth and the views given: the background sheet bids too), else footprints.
template <bool VS>
static void launch_triangles(int pass, int res, int K, int n_pts, int N, const InstTable& itab, const double* uvz, const float* depth,
                             float ratio, const ReprojectWs& w, const float* bg_depth, const Xf* views, hipStream_t st) {
  hipLaunchKernelGGL(k_fp_tri<VS>, dim3(cdiv(2 * (res - 1) * (res - 1), 256), K), dim3(256), 0, st, pass, res, n_pts, N, (const int*)w.inv,
                     itab, uvz, depth, ratio, fp_tier(), w.zbuf, w.owner, w.big_list, w.big_stride, w.big_count, bg_depth, views);
  hipLaunchKernelGGL(k_fp_wave<VS>, dim3(FP_WAVE_BLOCKS, K), dim3(256), 0, st, pass, res, n_pts, (const int*)w.inv, itab, uvz, depth, ratio,
                     w.zbuf, w.owner, w.big_list, w.big_stride, w.big_count, bg_depth, views);
}

// The harmonic in-fill of K images: the multi-workgroup solver, then the single-workgroup one; each takes the systems of its
// size class (multi_min: the smallest the first takes; holes beyond one CU's LDS go to CGM_WGS workgroups per image, beyond that
// kernel's register budget of 65 536 unknowns to the single-workgroup kernel).  Every polled word is zeroed per call.
struct CgScratch {
  double *vx, *vr, *vp, *vq;
  int* pixmap;
  int2 *nb_ud, *nb_lr;
  size_t ud_stride, lr_stride;
  CgSync* sync;
};
static int launch_infill(const CgScratch& s, int K, int res, float* x, const uint8_t* unknown, const int* unk, int* counts,
                         int max_iter, const float* rhs, int multi_min, int border, hipStream_t st) {
  DH_CHECK_HIP(hipMemsetAsync(s.sync, 0, (size_t)K * sizeof(CgSync), st));
  hipLaunchKernelGGL(k_cg_fill_multi, dim3(CGM_WGS, K), dim3(1024), 0, st, res, x, unknown, unk, counts, 4, 2, 3, s.vx, s.vr, s.vp,
                     s.vq, max_iter, 1e-24, counts, rhs, multi_min, s.pixmap, s.nb_ud, s.ud_stride, s.nb_lr, s.lr_stride, s.sync,
                     border);
  hipLaunchKernelGGL(k_cg_fill, dim3(K), dim3(1024), 0, st, res, x, unknown, unk, counts, 4, 2, 3, s.vx, s.vr, s.vp, s.vq, max_iter,
                     1e-24, counts, rhs, CGM_WGS * CGM_EPT * 1024, s.pixmap, s.nb_ud, s.ud_stride, s.nb_lr, s.lr_stride, border);
  return DH_OK;
}
// the scratch of the solve in a re-projection: the z-buffer, owner map and key list are dead by then (last read by k_pixels /
// k_write_corr)
static CgScratch reproject_cg_scratch(const ReprojectWs& w, size_t R2, size_t P) {
  return {w.vx, w.vr, w.vp, w.vq, w.owner, reinterpret_cast<int2*>(w.zbuf), reinterpret_cast<int2*>(w.key), R2, P, w.cgsync};
}

// n_objects masks: mask m owns fg_pix[obj_start[m] .. obj_start[m + 1]).  n_inst instances per edit: instance n draws the points
// of mask inst_obj[n] with row e * n_inst + n of xforms_host (DH_SIMILARITY_ROW doubles: rotation, translation, scale, pivot);
// the point list holds them one after the other (InstTable), n_pts foreground points in all.  Only k_centroid (masks) and
// k_points, the triangles and the row writers (instances) know about either; from the z-buffer on the point list is one list.
// The one code path of the re-projection with foreground points.  inst_obj = NULL with n_instances = 0: the call without copies
// (inst_obj[n] = n) with the workspace layout it always had -- dh_reproject_footprint_edits' and the entries' before it.
//
// footprints = 1 (point mode's footprint splatting): the triangles between neighbouring points of one INSTANCE bid in the same
// z-buffer, in both passes; vis, the kept set and the correspondences are then taken per TARGET pixel (corr_capacity rows per
// edit: res * res; without footprints n_pts).  max_ratio: 0 = none, else the depth-ratio guard of the triangles (finite, > 1).
static int reproject_instances(const dh_reproject_args& a) {
  const float *depth = a.depth, *bg_depth = a.bg_depth, *grid_x = a.grid_x, *grid_y = a.grid_y, *bounds = a.bounds;
  const float *donor_depth = a.donor_depth, *bone_w = a.bone_w;
  const int32_t *fg_pix = a.fg_pix, *obj_start = a.obj_start;
  const double* xforms_host = a.xforms_host;
  const uint8_t *has_view = a.has_view, *bg_valid = a.bg_valid;
  float *zmap = a.zmap, *disparity = a.disparity;
  uint8_t *raw_mask = a.raw_mask, *clean_mask = a.clean_mask, *vis = a.vis, *corr_inst = a.corr_inst;
  int32_t *target_xy = a.target_xy, *counts = a.counts, *bg_counts = a.bg_counts;
  int64_t *corr = a.corr, *bg_corr = a.bg_corr;
  const int res = a.res, n_fg = a.n_fg, n_objects = a.n_objects, n_edits = a.n_edits, corr_capacity = a.corr_capacity;
  const int footprints = a.footprints, infill_border = a.infill_border, view_surfaces = a.view_surfaces;
  const float inv_fx = a.inv_fx, inv_fy = a.inv_fy, max_ratio = a.max_ratio, surface_max_ratio = a.surface_max_ratio;
  const double fx = a.fx, fy = a.fy;
  // the identity table: N = M, instance n draws mask n, on the carving the footprint entry always had
  static const int32_t identity[MAX_OBJECTS] = {0, 1, 2, 3, 4, 5, 6, 7};
  const bool identity_carve = !a.inst_obj && a.n_instances == 0;
  const int32_t* inst_obj = identity_carve ? identity : a.inst_obj;
  const int n_inst = identity_carve ? n_objects : a.n_instances;
  // bend edits: n_bones rows per instance and edit (0 = 1: none); the weights stay on the device and are never read here
  const int n_bones = a.n_bones == 0 ? 1 : a.n_bones;
  DH_REQUIRE(n_bones >= 1 && n_bones <= DH_MAX_BONES, "n_bones must lie in 1 .. 4");
  DH_REQUIRE(n_bones == 1 || bone_w, "n_bones > 1 without bone_w");
  DH_REQUIRE((reinterpret_cast<uintptr_t>(bone_w) & 15u) == 0, "bone_w must be 16-byte aligned");
  DH_REQUIRE(infill_border == 0 || infill_border == 1, "infill_border must be 0 (zero) or 1 (reflect)");
  DH_REQUIRE(view_surfaces == 0 || view_surfaces == 1, "view_surfaces must be 0 or 1");
  DH_REQUIRE(surface_max_ratio == 0.f || (surface_max_ratio > 1.f && surface_max_ratio <= 3.4028234663852886e38f),
             "surface_max_ratio must be 0 (none) or finite and > 1");
  DH_REQUIRE(surface_max_ratio == 0.f || view_surfaces, "surface_max_ratio without view_surfaces");
  DH_REQUIRE(!(view_surfaces && footprints), "view_surfaces with footprints are not supported (footprints stay refused with a view)");
  DH_REQUIRE(depth && bg_depth && fg_pix && grid_x && grid_y && xforms_host && obj_start && inst_obj, "null input");
  DH_REQUIRE(zmap && raw_mask && clean_mask && disparity && vis && target_xy && corr && counts, "null output");
  DH_REQUIRE(res >= 2 && n_fg > 0 && n_edits >= 1, "bad sizes");
  DH_REQUIRE(n_objects >= 1 && n_objects <= MAX_OBJECTS, "1 to 8 objects");
  DH_REQUIRE(n_inst >= 1 && n_inst <= MAX_OBJECTS, "1 to 8 instances");
  DH_REQUIRE(footprints == 0 || footprints == 1, "footprints must be 0 or 1");
  // the donor: masks n_host_objects .. n_objects - 1, the last n_donor_objects, draw from donor_depth
  const int n_host_objects = n_objects - a.n_donor_objects;
  DH_REQUIRE(n_host_objects >= 0 && n_host_objects <= n_objects, "n_host_objects must lie in 0 .. n_objects");
  if (n_host_objects < n_objects) {
    DH_REQUIRE(donor_depth, "donor objects without a donor depth");
    DH_REQUIRE(!footprints, "footprints with a donor are not supported (two images share pixel indices)");
    DH_REQUIRE(corr_inst, "a donor needs the instance column (corr_inst)");
    DH_REQUIRE(!view_surfaces, "view_surfaces with a donor are not supported (two images share pixel indices)");
  }
  if (!donor_depth) donor_depth = depth;
  DH_REQUIRE(max_ratio == 0.f || (max_ratio > 1.f && max_ratio <= 3.4028234663852886e38f),
             "footprint max_ratio must be 0 (none) or finite and > 1");
  DH_REQUIRE(max_ratio == 0.f || footprints, "footprint max_ratio without footprints");
  DH_REQUIRE(obj_start[0] == 0 && obj_start[n_objects] == n_fg, "obj_start must run from 0 to n_fg");
  for (int m = 0; m < n_objects; ++m) DH_REQUIRE(obj_start[m] < obj_start[m + 1], "obj_start must increase (no empty object)");
  long long n_pts_ll = 0;
  unsigned named = 0;
  for (int n = 0; n < n_inst; ++n) {
    DH_REQUIRE(inst_obj[n] >= 0 && inst_obj[n] < n_objects, "inst_obj: an instance names a mask outside 0 .. n_objects - 1");
    named |= 1u << inst_obj[n];
    n_pts_ll += obj_start[inst_obj[n] + 1] - obj_start[inst_obj[n]];
  }
  DH_REQUIRE(named == (1u << n_objects) - 1u, "inst_obj: a mask without an instance (removing an object is not supported)");
  DH_REQUIRE((long long)res * res + n_pts_ll <= 2147483647LL, "res * res + n_pts does not fit the int owner map");
  DH_REQUIRE((long long)corr_capacity >= (footprints ? (long long)res * res : n_pts_ll),
             "correspondence capacity too small (n_fg rows per edit without footprints, res * res with)");
  // every row before any launch
  for (size_t r = 0; r < (size_t)n_edits * n_inst * n_bones; ++r) {
    const char* why;
    DH_REQUIRE(row_ok(xforms_host + r * DH_SIMILARITY_ROW, &why), why);
  }
  // camera moves: every view row before any launch; without a view in any edit the call is the call without the arguments
  bool views_ok = true;
  const double* view_host = view_rows(a.views, has_view, n_edits, &views_ok);
  DH_REQUIRE(views_ok, "view row: malformed (finite members, scale positive, has-pivot flag 0 or 1)");
  if (view_host) {
    DH_REQUIRE(!footprints, "footprints with a view are not supported");
    DH_REQUIRE(bg_valid && bg_corr && bg_counts, "a view needs bg_valid, bg_corr and bg_counts");
  }
  // view surfaces act only where an edit has a view: without one the call is the call without the setting
  const bool surfaces = view_host != nullptr && view_surfaces != 0;
  DH_REQUIRE(!surfaces || (long long)corr_capacity >= (long long)res * res,
             "correspondence capacity too small (res * res rows per edit with view surfaces)");
  hipStream_t st = (hipStream_t)a.stream;
  const int K = n_edits, M = n_objects, N = n_inst;
  const ObjTable tab = obj_table(M, obj_start, n_fg);
  int n_pts = 0;
  const InstTable itab = inst_table(N, inst_obj, obj_start, &n_pts);
  const int R2 = res * res, P = R2 + n_pts;
  Arena arena(a.workspace, a.workspace_bytes);
  ReprojectWs w;
  DH_REQUIRE(!(identity_carve && n_bones > 1), "bones need the instance carving");
  DH_REQUIRE(carve(arena, carve_spec(a, n_pts, view_host != nullptr), w), "workspace too small");
  const size_t corr_stride = (size_t)corr_capacity;
  if (view_host) DH_CHECK_HIP(hipMemcpyAsync(w.views, view_host, (size_t)K * sizeof(Xf), hipMemcpyHostToDevice, st));

  int2 hc[MAX_OFFS], ho[MAX_OFFS];
  const int kc = res / 50, ko = res / 250;
  DH_REQUIRE(kc * kc <= MAX_OFFS && kc >= 1, "unsupported resolution for the close kernel");
  const int nc = ellipse_offsets(kc, hc);
  const int no = ellipse_offsets(ko < 1 ? 1 : ko, ho);
  DH_CHECK_HIP(hipMemcpyAsync(w.offs_close, hc, nc * sizeof(int2), hipMemcpyHostToDevice, st));
  DH_CHECK_HIP(hipMemcpyAsync(w.offs_open, ho, no * sizeof(int2), hipMemcpyHostToDevice, st));
  DH_CHECK_HIP(hipMemcpyAsync(w.xf, xforms_host, (size_t)K * N * n_bones * sizeof(Xf), hipMemcpyHostToDevice, st));
  DH_CHECK_HIP(hipMemsetAsync(w.zbuf, 0xff, (size_t)K * R2 * sizeof(unsigned long long), st));
  DH_CHECK_HIP(hipMemsetAsync(w.owner, 0x7f, (size_t)K * R2 * sizeof(int), st));
  DH_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)K * 4 * sizeof(int), st));
  // minmax init: min slot = 0xffffffff, max slot = 0
  DH_CHECK_HIP(hipMemsetAsync(w.minmax, 0, (size_t)2 * K * sizeof(unsigned int), st));
  for (int e = 0; e < K; ++e) DH_CHECK_HIP(hipMemsetAsync(w.minmax + 2 * e, 0xff, sizeof(unsigned int), st));

  hipLaunchKernelGGL(k_centroid, dim3(M), dim3(CEN_CHUNK), 0, st, depth, donor_depth, n_host_objects, fg_pix, tab, res, grid_x,
                     grid_y, inv_fx, inv_fy, w.cen);
  // footprints: the triangles between an instance's points; view surfaces: those and the background sheet, in the edits with a
  // view (the vertex pointer is that of the first foreground point: see fp_setup).  Never both.
  auto triangle_pass = [&](int pass) {
    if (footprints) launch_triangles<false>(pass, res, K, n_pts, N, itab, w.uvz, depth, max_ratio, w, nullptr, nullptr, st);
    if (surfaces) launch_triangles<true>(pass, res, K, n_pts, N, itab, w.uvz + (size_t)R2 * 3, depth, surface_max_ratio, w, bg_depth, w.views, st);
  };
  if (surfaces || footprints) {
    DH_CHECK_HIP(hipMemsetAsync(w.inv, 0xff, (size_t)R2 * sizeof(int), st));
    DH_CHECK_HIP(hipMemsetAsync(w.big_count, 0, (size_t)K * sizeof(int), st));
    hipLaunchKernelGGL(k_fp_inverse, dim3(cdiv(n_fg, 256)), dim3(256), 0, st, fg_pix, n_fg, w.inv);
  }
  // (the carving leaves uvz null without triangles and views null without a view, footprints included: they never meet a view)
  launch_points(footprints != 0, surfaces, bone_w != nullptr, dim3(cdiv(P, 256), K), st, depth, donor_depth, n_host_objects, bg_depth,
                fg_pix, n_pts, res, grid_x, grid_y, inv_fx, inv_fy, fx, fy, w.xf, w.cen, itab, N, w.zbuf, w.pix, w.key, w.uvz,
                w.views, bone_w, bone_w ? n_bones : 1);
  triangle_pass(1);
  hipLaunchKernelGGL(k_resolve, dim3(cdiv(P, 256), K), dim3(256), 0, st, P, R2, w.zbuf, w.pix, w.key, w.owner);
  triangle_pass(2);
  hipLaunchKernelGGL(k_pixels, dim3(cdiv(R2, 256 * PIX_PER_THREAD), K), dim3(256), 0, st, R2, w.zbuf, w.owner, zmap, raw_mask,
                     disparity, w.minmax, (const Xf*)w.views);
  hipLaunchKernelGGL(k_fg_vis, dim3(cdiv(n_pts, 256), K), dim3(256), 0, st, n_pts, R2, P, res, w.pix, w.owner, vis,
                     target_xy);
  // CLOSE = dilate, erode ; OPEN = erode, dilate
  if (res % 32 == 0 && kc < 32 && ko < 32) {        // bit rows: pack, four passes (erode = NOT dilate NOT), unpack
    const int nw = K * R2 / 32, wpe = R2 / 32;
    unsigned* ba = reinterpret_cast<unsigned*>(w.tmp_a);
    unsigned* bb = reinterpret_cast<unsigned*>(w.tmp_b);
    hipLaunchKernelGGL(k_pack_bits, dim3(cdiv(nw, 256)), dim3(256), 0, st, raw_mask, ba, nw);
    hipLaunchKernelGGL(k_morph_bits, dim3(cdiv(wpe, 256), K), dim3(256), 0, st, ba, bb, res, w.offs_close, nc, 0, 0);
    hipLaunchKernelGGL(k_morph_bits, dim3(cdiv(wpe, 256), K), dim3(256), 0, st, bb, ba, res, w.offs_close, nc, 1, 1);
    hipLaunchKernelGGL(k_morph_bits, dim3(cdiv(wpe, 256), K), dim3(256), 0, st, ba, bb, res, w.offs_open, no, 1, 1);
    hipLaunchKernelGGL(k_morph_bits, dim3(cdiv(wpe, 256), K), dim3(256), 0, st, bb, ba, res, w.offs_open, no, 0, 0);
    hipLaunchKernelGGL(k_unpack_bits, dim3(cdiv(nw, 256)), dim3(256), 0, st, ba, clean_mask, nw);
  } else {
    hipLaunchKernelGGL(k_morph, dim3(cdiv(R2, 256), K), dim3(256), 0, st, raw_mask, w.tmp_a, res, w.offs_close, nc, 1);
    hipLaunchKernelGGL(k_morph, dim3(cdiv(R2, 256), K), dim3(256), 0, st, w.tmp_a, w.tmp_b, res, w.offs_close, nc, 0);
    hipLaunchKernelGGL(k_morph, dim3(cdiv(R2, 256), K), dim3(256), 0, st, w.tmp_b, w.tmp_a, res, w.offs_open, no, 0);
    hipLaunchKernelGGL(k_morph, dim3(cdiv(R2, 256), K), dim3(256), 0, st, w.tmp_a, clean_mask, res, w.offs_open, no, 1);
  }
  if (footprints) {
    // per TARGET pixel: vis = the point owns a pixel, keep = foreground-owned and inside the cleaned mask.  The flags and the
    // compacted list live in the in-fill's buffers (inpaint / unk: written again further down, after the rows are out)
    DH_CHECK_HIP(hipMemsetAsync(vis, 0, (size_t)K * n_pts, st));
    hipLaunchKernelGGL(k_fp_vis, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, n_pts, w.owner, raw_mask, vis, clean_mask, w.inpaint);
    compact(w.inpaint, R2, K, R2, w.unk, R2, counts + 0, 4, w.block_counts, st);
    hipLaunchKernelGGL(k_write_corr_target, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, res, fg_pix, itab, w.owner, w.unk, counts,
                       4, corr_stride, (long long*)corr, corr_inst);
  } else {
    hipLaunchKernelGGL(k_keep_flags, dim3(cdiv(n_pts, 256), K), dim3(256), 0, st, n_pts, R2, P, w.pix, vis, clean_mask,
                       w.keep, surfaces ? (const Xf*)w.views : (const Xf*)nullptr);
    compact(w.keep, n_pts, K, n_pts, w.keep_idx, n_pts, counts + 0, 4, w.block_counts, st);
    hipLaunchKernelGGL(k_write_corr, dim3(cdiv(n_pts, 256), K), dim3(256), 0, st, n_pts, res, fg_pix, itab, target_xy,
                       w.keep_idx, counts, 4, corr_stride, (long long*)corr, corr_inst);
  }
  if (surfaces) {
    // the edits with a view: vis again (a point is visible when it owns a pixel), then the rows per TARGET pixel, the
    // instances' and the background's.  Flags and lists live in the morphology's and the in-fill's buffers (tmp_a: dead;
    // inpaint / unk: written again further down); the row counts of the target pass in the wave tier's counter (dead).
    for (int e = 0; e < K; ++e)
      if (has_view[e]) DH_CHECK_HIP(hipMemsetAsync(vis + (size_t)e * n_pts, 0, (size_t)n_pts, st));
    hipLaunchKernelGGL(k_vs_flags, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, n_pts, w.owner, clean_mask, (size_t)R2, bg_valid,
                       (const Xf*)w.views, vis, w.inpaint, w.tmp_a);
    compact(w.inpaint, R2, K, R2, w.unk, R2, w.big_count, 1, w.block_counts, st);
    hipLaunchKernelGGL(k_write_corr_target, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, res, fg_pix, itab, w.owner, w.unk,
                       w.big_count, 1, corr_stride, (long long*)corr, corr_inst);
    hipLaunchKernelGGL(k_vs_add_counts, dim3(cdiv(K, 64)), dim3(64), 0, st, K, w.big_count, counts);
    compact(w.tmp_a, R2, K, R2, w.unk, R2, bg_counts, 1, w.block_counts, st);
    hipLaunchKernelGGL(k_vs_write_bg, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, res, w.owner, w.unk, bg_counts,
                       (long long*)bg_corr);
  }
  hipLaunchKernelGGL(k_count_flags, dim3(cdiv(n_pts, 256), K), dim3(256), 0, st, vis, n_pts, counts, 4, 1);
  if (w.views && !surfaces) {
    // the background rows: flags and the compacted list live in the in-fill's buffers (inpaint / unk: written just below)
    hipLaunchKernelGGL(k_bg_row_flags, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, P, w.pix, w.owner, clean_mask, (size_t)R2,
                       bg_valid, (const Xf*)w.views, w.inpaint);
    compact(w.inpaint, R2, K, R2, w.unk, R2, bg_counts, 1, w.block_counts, st);
    hipLaunchKernelGGL(k_write_bg_corr, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, P, res, w.pix, w.unk, bg_counts,
                       (long long*)bg_corr);
  }
  hipLaunchKernelGGL(k_normalize, dim3(cdiv(R2, 256), K), dim3(256), 0, st, R2, disparity, w.minmax, bounds, raw_mask,
                     clean_mask, w.inpaint, w.zbuf, (const Xf*)w.views);
  compact(w.inpaint, R2, K, R2, w.unk, R2, counts + 2, 4, w.block_counts, st);
#ifdef DH_TUNING
  static const bool cg_lds = !(getenv("DH_CG_LDS") && atoi(getenv("DH_CG_LDS")) == 0);
#else
  constexpr bool cg_lds = true;
#endif
  const int rc = launch_infill(reproject_cg_scratch(w, R2, P), K, res, disparity, w.inpaint, w.unk, counts, cg_cap(20000), nullptr,
                               cg_lds ? CG_SLOTS * 1024 : 0, infill_border, st);
  if (rc != DH_OK) return rc;
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// Object removal, the pure case (no foreground point left): the background part of the point list through the kernels of
// reproject_instances -- k_points (n_pts = 0: every thread takes the background branch), k_resolve, k_pixels, k_normalize, the
// in-fill solvers -- on the carving of a one-edit call without foreground.  Nothing is foreground, so raw and cleaned masks are
// zero and stay in the workspace; the in-fill set is the pixels no point owns (k_unowned in the raw mask's place).
//
// Camera moves, the pure case: with a view row (has_view[0]; none = the pure removal, launch for launch) the view lives in the
// one transform row the carving holds and the background never reads; the points go through k_points' view path (no clamp:
// points out of frame bid for nothing), the pixels no point reached stay out of the min / max, and every owned background point
// with bg_valid != 0 yields a row (bg_corr [res * res][4], bg_counts [1]).  infill_border: the border rule of the harmonic
// in-fill.  view_surfaces with a view: the two triangles of every source quad bid beside the points (surface_max_ratio: their
// depth-ratio guard), and the rows are one per target pixel whose owner has bg_valid, row-major.
//
// A launch sequence of its own: no morphology, k_unowned.  Its refusals carry the name of the entry it was written as.
#define BG_REQUIRE(cond, msg) DH_REQUIRE_AS("dh_reproject_surface_background", cond, msg)
static int reproject_background(const dh_reproject_args& a) {
  const float *bg_depth = a.bg_depth, *grid_x = a.grid_x, *grid_y = a.grid_y;
  float *zmap = a.zmap, *disparity = a.disparity;
  int32_t *counts = a.counts, *bg_counts = a.bg_counts;
  const int res = a.res;
  BG_REQUIRE(a.infill_border == 0 || a.infill_border == 1, "infill_border must be 0 (zero) or 1 (reflect)");
  BG_REQUIRE(a.view_surfaces == 0 || a.view_surfaces == 1, "view_surfaces must be 0 or 1");
  BG_REQUIRE(a.surface_max_ratio == 0.f || (a.surface_max_ratio > 1.f && a.surface_max_ratio <= 3.4028234663852886e38f),
             "surface_max_ratio must be 0 (none) or finite and > 1");
  BG_REQUIRE(a.surface_max_ratio == 0.f || a.view_surfaces, "surface_max_ratio without view_surfaces");
  BG_REQUIRE(bg_depth && grid_x && grid_y, "null input");
  BG_REQUIRE(zmap && disparity && counts && a.workspace, "null output");
  BG_REQUIRE(res >= 2 && res <= 32768, "bad sizes");
  BG_REQUIRE(a.n_edits == 1, "the call without a foreground point takes one edit");
  bool view_ok = true;
  const double* view_host = view_rows(a.views, a.has_view, 1, &view_ok);
  BG_REQUIRE(view_ok, "view row: malformed (finite members, scale positive, has-pivot flag 0 or 1)");
  if (view_host) BG_REQUIRE(a.bg_valid && a.bg_corr && bg_counts, "a view needs bg_valid, bg_corr and bg_counts");
  hipStream_t st = (hipStream_t)a.stream;
  const int R2 = res * res;
  Arena arena(a.workspace, a.workspace_bytes);
  ReprojectWs w;
  const CarveSpec spec = carve_spec(a, 0, view_host != nullptr);
  const bool surfaces = spec.surfaces;
  BG_REQUIRE(carve(arena, spec, w), "workspace too small");
  const Xf* dview = nullptr;
  if (view_host) {
    DH_CHECK_HIP(hipMemcpyAsync(w.xf, view_host, sizeof(Xf), hipMemcpyHostToDevice, st));
    dview = w.xf;
  }
  const int32_t none[2] = {0, 0};
  int n_pts = 0;
  const InstTable itab = inst_table(0, none, none, &n_pts);
  DH_CHECK_HIP(hipMemsetAsync(w.zbuf, 0xff, (size_t)R2 * sizeof(unsigned long long), st));
  DH_CHECK_HIP(hipMemsetAsync(w.owner, 0x7f, (size_t)R2 * sizeof(int), st));
  DH_CHECK_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int), st));
  DH_CHECK_HIP(hipMemsetAsync(w.minmax, 0, 2 * sizeof(unsigned int), st));
  DH_CHECK_HIP(hipMemsetAsync(w.minmax, 0xff, sizeof(unsigned int), st));
  DH_CHECK_HIP(hipMemsetAsync(w.tmp_b, 0, (size_t)R2, st));
  auto surface_pass = [&](int pass) {          // the background sheet alone: no instance, the vertex pointer past the R2 points
    launch_triangles<true>(pass, res, 1, 0, 0, itab, w.uvz + (size_t)R2 * 3, bg_depth, a.surface_max_ratio, w, bg_depth, dview, st);
  };
  if (surfaces) DH_CHECK_HIP(hipMemsetAsync(w.big_count, 0, sizeof(int), st));
  launch_points(false, surfaces, false, dim3(cdiv(R2, 256), 1), st, bg_depth, bg_depth, 0, bg_depth, nullptr, 0, res, grid_x, grid_y,
                a.inv_fx, a.inv_fy, a.fx, a.fy, w.xf, w.cen, itab, 0, w.zbuf, w.pix, w.key, w.uvz, dview, nullptr, 1);
  if (surfaces) surface_pass(1);
  hipLaunchKernelGGL(k_resolve, dim3(cdiv(R2, 256), 1), dim3(256), 0, st, R2, R2, w.zbuf, w.pix, w.key, w.owner);
  if (surfaces) surface_pass(2);
  hipLaunchKernelGGL(k_pixels, dim3(cdiv(R2, 256 * PIX_PER_THREAD), 1), dim3(256), 0, st, R2, w.zbuf, w.owner, zmap, w.tmp_a,
                     disparity, w.minmax, dview);
  if (surfaces) {
    hipLaunchKernelGGL(k_vs_flags, dim3(cdiv(R2, 256), 1), dim3(256), 0, st, R2, 0, w.owner, w.tmp_b, (size_t)0, a.bg_valid, dview,
                       (uint8_t*)nullptr, (uint8_t*)nullptr, w.inpaint);
    compact(w.inpaint, R2, 1, R2, w.unk, R2, bg_counts, 1, w.block_counts, st);
    hipLaunchKernelGGL(k_vs_write_bg, dim3(cdiv(R2, 256), 1), dim3(256), 0, st, R2, res, w.owner, w.unk, bg_counts,
                       (long long*)a.bg_corr);
  } else if (dview) {
    hipLaunchKernelGGL(k_bg_row_flags, dim3(cdiv(R2, 256), 1), dim3(256), 0, st, R2, R2, w.pix, w.owner, w.tmp_b, (size_t)0, a.bg_valid,
                       dview, w.inpaint);
    compact(w.inpaint, R2, 1, R2, w.unk, R2, bg_counts, 1, w.block_counts, st);
    hipLaunchKernelGGL(k_write_bg_corr, dim3(cdiv(R2, 256), 1), dim3(256), 0, st, R2, R2, res, w.pix, w.unk, bg_counts,
                       (long long*)a.bg_corr);
  }
  hipLaunchKernelGGL(k_unowned, dim3(cdiv(R2, 256)), dim3(256), 0, st, R2, w.zbuf, w.tmp_a);
  hipLaunchKernelGGL(k_normalize, dim3(cdiv(R2, 256), 1), dim3(256), 0, st, R2, disparity, w.minmax, a.bounds, w.tmp_a, w.tmp_b,
                     w.inpaint, w.zbuf, dview);
  compact(w.inpaint, R2, 1, R2, w.unk, R2, counts + 2, 4, w.block_counts, st);
  const int rc = launch_infill(reproject_cg_scratch(w, R2, R2), 1, res, disparity, w.inpaint, w.unk, counts, cg_cap(20000), nullptr,
                               CG_SLOTS * 1024, a.infill_border, st);
  if (rc != DH_OK) return rc;
  DH_LAUNCH_CHECK();
  return DH_OK;
}

#undef BG_REQUIRE

// what every workspace query answers: the end of a carving in a null-based arena, and the slack behind it
template <class F>
static size_t carved_bytes(F carve_into) {
  Arena a(nullptr, (size_t)-1);
  carve_into(a);
  return a.off + 256;
}

// The two entries of the re-projection (include/diffhandles_hip.h, dh_reproject_args).  Every positional dh_reproject_* entry
// and query is a record filled in csrc/reproject_compat.cpp.
extern "C" int dh_reproject(const dh_reproject_args* a) {
  DH_REQUIRE(a && a->struct_bytes == sizeof(dh_reproject_args), "struct_bytes is not sizeof(dh_reproject_args)");
  return a->n_fg == 0 ? reproject_background(*a) : reproject_instances(*a);
}

extern "C" int dh_reproject_workspace(const dh_reproject_args* a, size_t* bytes) {
  DH_REQUIRE(a && a->struct_bytes == sizeof(dh_reproject_args), "struct_bytes is not sizeof(dh_reproject_args)");
  DH_REQUIRE(a->res >= 2 && a->n_fg >= 0 && a->n_edits >= 1 && a->n_objects >= (a->n_fg > 0 ? 1 : 0) && a->n_objects <= MAX_OBJECTS && bytes,
             "bad arguments");
  const bool table = a->inst_obj || a->n_instances;
  DH_REQUIRE(!table || (a->n_instances >= 1 && a->n_instances <= MAX_OBJECTS), "1 to 8 instances");
  DH_REQUIRE(a->view_surfaces == 0 || a->view_surfaces == 1, "view_surfaces must be 0 or 1");
  DH_REQUIRE(a->footprints == 0 || a->footprints == 1, "footprints must be 0 or 1");
  DH_REQUIRE(!(a->footprints && a->view_surfaces), "view_surfaces with footprints are not supported");
  DH_REQUIRE(a->n_bones >= 0 && a->n_bones <= DH_MAX_BONES, "n_bones must lie in 1 .. 4");
  long long n_pts = a->n_fg;
  if (a->inst_obj && a->obj_start) {          // the points of the instances, as the call counts them
    n_pts = 0;
    for (int n = 0; n < a->n_instances; ++n) {
      DH_REQUIRE(a->inst_obj[n] >= 0 && a->inst_obj[n] < a->n_objects, "inst_obj: an instance names a mask outside 0 .. n_objects - 1");
      n_pts += a->obj_start[a->inst_obj[n] + 1] - a->obj_start[a->inst_obj[n]];
    }
    DH_REQUIRE(n_pts >= 0 && n_pts <= 2147483647LL, "bad arguments");
  }
  bool any_view = false;
  for (int e = 0; a->has_view && e < a->n_edits; ++e) any_view = any_view || a->has_view[e] != 0;
  const CarveSpec spec = carve_spec(*a, (int)n_pts, any_view);
  *bytes = carved_bytes([&](Arena& arena) {
    ReprojectWs w;
    carve(arena, spec, w);
  });
  return DH_OK;
}

namespace dh {
struct BlendWs {
  double *vx, *vr, *vp, *vq;
  uint8_t *m0, *m1;
  float* lap;
  int *unk, *pixmap;
  int2 *nb_ud, *nb_lr;
  int* bc;
  CgSync* cgs;
};
static bool carve_blend(Arena& a, int res, BlendWs& w) {
  const size_t R2 = (size_t)res * res;
  w.vx = a.take<double>(R2); w.vr = a.take<double>(R2); w.vp = a.take<double>(R2); w.vq = a.take<double>(R2);
  w.m0 = a.take<uint8_t>(R2); w.m1 = a.take<uint8_t>(R2);
  w.lap = a.take<float>(R2);
  w.unk = a.take<int>(R2);
  w.pixmap = a.take<int>(R2);
  w.nb_ud = a.take<int2>(R2);
  w.nb_lr = a.take<int2>(R2);
  w.bc = a.take<int>(cdiv((int)R2, CP_TILE) + 2);
  w.cgs = a.take<CgSync>(1);
  return a.ok();
}
}  // namespace dh

extern "C" int dh_laplacian_blend_workspace_bytes(int res, size_t* bytes) {
  DH_REQUIRE(res >= 2 && bytes, "bad arguments");
  *bytes = carved_bytes([&](Arena& a) {
    BlendWs w;
    carve_blend(a, res, w);
  });
  return DH_OK;
}

// DiffusionHandles.set_foreground (diffusion_handles.py:90-111) = utils.solve_laplacian_depth (utils.py:49-102)
// over binary_dilation(fg_mask, iterations): out = depth outside the dilated mask, inside the solution of
// 4 x - sum(masked nbrs) = sum(known depth nbrs) - laplacian(bg_depth).
// infill_border = 1 (reflect): the diagonal is the in-image degree and the Laplacian of bg_depth uses replicate padding, so
// depth == bg_depth on the ring still gives out == bg_depth inside.  The workspace is dh_laplacian_blend_workspace_bytes'.
extern "C" int dh_laplacian_blend_border(const float* depth, const float* bg_depth, const uint8_t* fg_mask, int res,
                                         int dilate_iters, float* out, int32_t* counts, void* workspace,
                                         size_t workspace_bytes, void* stream, int infill_border) {
  DH_REQUIRE(infill_border == 0 || infill_border == 1, "infill_border must be 0 (zero) or 1 (reflect)");
  DH_REQUIRE(depth && bg_depth && fg_mask && out && counts && workspace && res >= 2 && dilate_iters >= 0, "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int R2 = res * res;
  Arena a(workspace, workspace_bytes);
  BlendWs w;
  DH_REQUIRE(carve_blend(a, res, w), "workspace too small");
  DH_CHECK_HIP(hipMemcpyAsync(w.m0, fg_mask, R2, hipMemcpyDeviceToDevice, st));
  uint8_t *src = w.m0, *dst = w.m1;
  for (int i = 0; i < dilate_iters; ++i) {
    hipLaunchKernelGGL(k_dilate_cross, dim3(cdiv(R2, 256)), dim3(256), 0, st, src, dst, res);
    uint8_t* t = src; src = dst; dst = t;
  }
  hipLaunchKernelGGL(k_laplacian, dim3(cdiv(R2, 256)), dim3(256), 0, st, bg_depth, w.lap, res, infill_border);
  DH_CHECK_HIP(hipMemcpyAsync(out, depth, (size_t)R2 * 4, hipMemcpyDeviceToDevice, st));
  DH_CHECK_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int), st));
  compact(src, R2, 1, 0, w.unk, 0, counts + 2, 1, w.bc, st);
  const CgScratch scratch = {w.vx, w.vr, w.vp, w.vq, w.pixmap, w.nb_ud, w.nb_lr, (size_t)R2, (size_t)R2, w.cgs};
  const int rc = launch_infill(scratch, 1, res, out, src, w.unk, counts, cg_cap(50000), w.lap, CG_SLOTS * 1024, infill_border, st);
  if (rc != DH_OK) return rc;
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// the call with the zero border
extern "C" int dh_laplacian_blend(const float* depth, const float* bg_depth, const uint8_t* fg_mask, int res,
                                  int dilate_iters, float* out, int32_t* counts, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return dh_laplacian_blend_border(depth, bg_depth, fg_mask, res, dilate_iters, out, counts, workspace, workspace_bytes, stream, 0);
}
