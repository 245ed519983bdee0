// Correspondences -> grid x grid cell index lists (integer work, bit-exact vs
// oracle/guidance_ref.py::cells_from_correspondences, which is pinned to the reference's
// GuidedStableDiffuser.process_correspondences, guided_stable_diffuser.py:490-584).
#include "common.h"
#include "compact.h"

namespace dh {

__global__ void k_valid(const long long* corr, int n, int img_res, uint8_t* valid) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long tx = corr[4 * (size_t)i + 2], ty = corr[4 * (size_t)i + 3];
  valid[i] = (tx >= 0 && tx < img_res && ty >= 0 && ty < img_res) ? 1 : 0;
}

__global__ void k_init_masks(uint8_t* m, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) m[i] = 1;
}

// row_donor (dh_cells_from_correspondences_donor): NULL, or one byte per correspondence row; a flagged row's source cell lies in
// another image, so it forms its pair and clears its target cell but leaves the original-background mask alone.
// three_kinds (dh_cells_from_correspondences_rows): the byte is the row's KIND -- 0 a host row, 1 a donor row, 2 a background
// row of a camera move, which forms its pair and clears NEITHER mask (the background stays background on both sides).
__global__ void k_pairs(const long long* corr, const int* idx, const int* count, int img_res, int grid, int* pairs,
                        uint8_t* bg_o, uint8_t* bg_t, const uint8_t* row_donor, int three_kinds) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= *count) return;
  const int row = idx[r];
  const long long* c = corr + 4 * (size_t)row;
  const int cs = img_res / grid;
  int oc = (int)(c[1] / cs) * grid + (int)(c[0] / cs);
  int tc = (int)(c[3] / cs) * grid + (int)(c[2] / cs);
  pairs[2 * (size_t)r + 0] = oc;
  pairs[2 * (size_t)r + 1] = tc;
  const int kind = row_donor ? row_donor[row] : 0;
  if (kind == 0) bg_o[oc] = 0;
  if (!(three_kinds && kind == 2)) bg_t[tc] = 0;
}

// object removal (dh_cells_from_correspondences_vacated): a cell that holds a vacated pixel leaves the original-background mask,
// as if a kept correspondence started in it (one thread per pixel; racing byte stores all write 0)
__global__ void k_vacated_cells(const uint8_t* vacated, int img_res, int grid, uint8_t* bg_o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= img_res * img_res) return;
  if (vacated[i]) {
    const int cs = img_res / grid, y = i / img_res, x = i - y * img_res;
    bg_o[(y / cs) * grid + x / cs] = 0;
  }
}

// scipy.ndimage.binary_erosion: cross structuring element, border_value 0, `iters` passes.
// blockIdx.x selects the mask (0 = orig, 1 = trans); one workgroup per mask, ping-pong in LDS.
__global__ void __launch_bounds__(1024) k_erode(uint8_t* masks, int grid, int iters) {
  extern __shared__ uint8_t sm[];
  const int n = grid * grid;
  uint8_t* m = masks + (size_t)blockIdx.x * n;
  uint8_t* a = sm;
  uint8_t* b = sm + n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) a[i] = m[i];
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int y = i / grid, x = i - y * grid;
      bool v = a[i] && y > 0 && y < grid - 1 && x > 0 && x < grid - 1;
      if (v) v = a[i - grid] && a[i + grid] && a[i - 1] && a[i + 1];
      b[i] = v ? 1 : 0;
    }
    __syncthreads();
    uint8_t* t = a; a = b; b = t;
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) m[i] = a[i];
}

// masks layout in: [orig][trans]; out layout [both][orig][trans]
__global__ void k_three_masks(const uint8_t* two, uint8_t* three, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t o = two[i], t = two[n + i];
  three[i] = o & t;
  three[n + i] = o;
  three[2 * n + i] = t;
}

// ---- keep map of the background lock (dh_keep_map) ---------------------------------------------------------------------
// region [s*s] u8, zeroed by the entry: 1 where a cell holds a non-zero pixel of the mask or of the release image (one
// thread per pixel; racing byte stores all write 1) ...
__global__ void k_keep_region_pixels(const uint8_t* mask, const uint8_t* release, int res, int s, uint8_t* region) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= res * res) return;
  if ((mask && mask[i]) || (release && release[i])) {
    const int cs = res / s, y = i / res, x = i - y * res;
    region[(y / cs) * s + x / cs] = 1;
  }
}

// ... or a correspondence's source pixel, or its target pixel when that lies in the image
__global__ void k_keep_region_corr(const long long* corr, int n, int res, int s, uint8_t* region) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long* c = corr + 4 * (size_t)i;
  const int cs = res / s;
  if (c[0] >= 0 && c[0] < res && c[1] >= 0 && c[1] < res) region[(int)(c[1] / cs) * s + (int)(c[0] / cs)] = 1;
  if (c[2] >= 0 && c[2] < res && c[3] >= 0 && c[3] < res) region[(int)(c[3] / cs) * s + (int)(c[2] / cs)] = 1;
}

// one thread per cell: d = Chebyshev distance to the nearest region cell inside the window of dilate + feather + 1 cells,
// clipped by the border; keep = 0 for d <= dilate, (d - dilate) / (feather + 1) up to the window's edge, 1 beyond it
__global__ void k_keep_distance(const uint8_t* region, int s, int dilate, int feather, float* keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s * s) return;
  const int y = i / s, x = i - y * s;
  const int R = dilate + feather + 1;
  const int y0 = max(y - R, 0), y1 = min(y + R, s - 1), x0 = max(x - R, 0), x1 = min(x + R, s - 1);
  int d = R + 1;
  for (int yy = y0; yy <= y1; ++yy) {
    const int dy = abs(yy - y);
    if (dy >= d) continue;
    const uint8_t* row = region + (size_t)yy * s;
    for (int xx = x0; xx <= x1; ++xx)
      if (row[xx]) d = min(d, max(dy, abs(xx - x)));
  }
  float k = 1.f;
  if (d <= dilate) k = 0.f;
  else if (d <= R) k = fminf(1.f, (float)(d - dilate) / (float)(feather + 1));
  keep[i] = k;
}

}  // namespace dh

using namespace dh;

extern "C" int dh_keep_map(const int64_t* corr, int n, const uint8_t* mask, const uint8_t* release, int res, int s, int dilate,
                           int feather, float* keep, void* workspace, size_t workspace_bytes, void* stream) {
  DH_REQUIRE(keep && workspace && n >= 0 && (n == 0 || corr), "bad arguments");
  DH_REQUIRE(s >= 1 && s <= 4096 && res >= s && res <= 32768 && res % s == 0, "res must be a multiple of s");
  DH_REQUIRE(dilate >= 0 && feather >= 0 && dilate + feather <= 31, "dilate, feather >= 0 and dilate + feather <= 31");
  DH_REQUIRE(workspace_bytes >= (size_t)s * s, "workspace too small (s * s bytes)");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* region = (uint8_t*)workspace;
  DH_CHECK_HIP(hipMemsetAsync(region, 0, (size_t)s * s, st));
  if (mask || release)
    hipLaunchKernelGGL(k_keep_region_pixels, dim3(cdiv(res * res, 256)), dim3(256), 0, st, mask, release, res, s, region);
  if (n > 0)
    hipLaunchKernelGGL(k_keep_region_corr, dim3(cdiv(n, 256)), dim3(256), 0, st, (const long long*)corr, n, res, s, region);
  hipLaunchKernelGGL(k_keep_distance, dim3(cdiv(s * s, 256)), dim3(256), 0, st, region, s, dilate, feather, keep);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

namespace dh {
struct CellsWs {
  uint8_t *valid, *two;
  int *idx, *bc;
};
static bool carve_cells(Arena& a, int n, int grid, CellsWs& w) {
  const size_t nn = n > 0 ? n : 1, G2 = (size_t)grid * grid;
  w.valid = a.take<uint8_t>(nn);
  w.idx = a.take<int>(nn);
  w.two = a.take<uint8_t>(2 * G2);
  w.bc = a.take<int>(3 * (size_t)(cdiv((int)nn, CP_TILE) + cdiv((int)G2, CP_TILE) + 2));
  return a.ok();
}
}  // namespace dh

extern "C" int dh_cells_workspace_bytes(int n, int grid, size_t* bytes) {
  DH_REQUIRE(n >= 0 && grid >= 1 && bytes, "bad arguments");
  Arena a(nullptr, (size_t)-1);
  CellsWs w;
  carve_cells(a, n, grid, w);
  *bytes = a.off + 256;
  return DH_OK;
}

// vacated: NULL, or the [img_res][img_res] image of the pixels an edit's removed objects leave behind (non-zero = vacated); its
// cells are cleared from the original-background mask between k_pairs and k_erode, so the erosion pushes the background away
// from them as it does from an object.  The transformed-background mask and the pairs do not see it.  n == 0 with an image is
// the pure removal.  NULL launches what dh_cells_from_correspondences always launched.
// row_donor: NULL, or [n] u8 on the device, one byte per correspondence row (non-zero = the row's source pixel lies in a donor
// image): such a row keeps its pair and clears its target cell, and does not clear a cell of the original-background mask.
// NULL or all zero gives the bytes of the _vacated entry, with the same launches.
// row_kind (dh_cells_from_correspondences_rows): NULL, or [n] u8 on the device: 0 = a host row, 1 = a donor row, 2 = a background
// row (camera moves): it forms its pair and clears neither mask.  The _donor entry is this code with the byte read as a flag
// (any non-zero value = a donor row), so kinds 0 and 1 give its bytes with its launches.
static int cells_rows(const int64_t* corr, int n, int img_res, int grid, int bg_erosion, int32_t* pairs, int32_t* bg_lists,
                      uint8_t* bg_masks, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream,
                      const uint8_t* vacated, const uint8_t* row_donor, int three_kinds) {
  DH_REQUIRE(pairs && bg_lists && bg_masks && counts && workspace, "null pointer");
  DH_REQUIRE(n >= 0 && grid >= 1 && img_res >= grid && img_res % grid == 0, "bad sizes");
  DH_REQUIRE(n == 0 || corr, "null corr");
  DH_REQUIRE(!vacated || img_res <= 32768, "img_res too large for a vacated image");
  DH_REQUIRE(2 * grid * grid <= 60000, "grid too large for the erosion kernel");
  hipStream_t st = (hipStream_t)stream;
  const int G2 = grid * grid;
  Arena a(workspace, workspace_bytes);
  CellsWs w;
  DH_REQUIRE(carve_cells(a, n, grid, w), "workspace too small");
  uint8_t *valid = w.valid, *two = w.two;
  int *idx = w.idx, *bc = w.bc;
  DH_CHECK_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int), st));
  hipLaunchKernelGGL(k_init_masks, dim3(cdiv(2 * G2, 256)), dim3(256), 0, st, two, 2 * G2);
  if (n > 0) {
    hipLaunchKernelGGL(k_valid, dim3(cdiv(n, 256)), dim3(256), 0, st, (const long long*)corr, n, img_res, valid);
    compact(valid, n, 1, 0, idx, 0, counts, 1, bc, st);
    hipLaunchKernelGGL(k_pairs, dim3(cdiv(n, 256)), dim3(256), 0, st, (const long long*)corr, idx, counts, img_res,
                       grid, pairs, two, two + G2, row_donor, three_kinds);
  }
  if (vacated)
    hipLaunchKernelGGL(k_vacated_cells, dim3(cdiv(img_res * img_res, 256)), dim3(256), 0, st, vacated, img_res, grid, two);
  if (bg_erosion > 0)
    hipLaunchKernelGGL(k_erode, dim3(2), dim3(1024), 2 * G2, st, two, grid, bg_erosion);
  hipLaunchKernelGGL(k_three_masks, dim3(cdiv(G2, 256)), dim3(256), 0, st, two, bg_masks, G2);
  compact(bg_masks, G2, 3, G2, bg_lists, G2, counts + 1, 1, bc, st);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_cells_from_correspondences_rows(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                                  int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                                  void* workspace, size_t workspace_bytes, void* stream,
                                                  const uint8_t* vacated, const uint8_t* row_kind) {
  return cells_rows(corr, n, img_res, grid, bg_erosion, pairs, bg_lists, bg_masks, counts, workspace, workspace_bytes, stream,
                    vacated, row_kind, 1);
}

extern "C" int dh_cells_from_correspondences_donor(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                                   int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                                   void* workspace, size_t workspace_bytes, void* stream,
                                                   const uint8_t* vacated, const uint8_t* row_donor) {
  return cells_rows(corr, n, img_res, grid, bg_erosion, pairs, bg_lists, bg_masks, counts, workspace, workspace_bytes, stream,
                    vacated, row_donor, 0);
}

extern "C" int dh_cells_from_correspondences_vacated(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                                     int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                                     void* workspace, size_t workspace_bytes, void* stream,
                                                     const uint8_t* vacated) {
  return dh_cells_from_correspondences_donor(corr, n, img_res, grid, bg_erosion, pairs, bg_lists, bg_masks, counts, workspace,
                                             workspace_bytes, stream, vacated, nullptr);
}

extern "C" int dh_cells_from_correspondences(const int64_t* corr, int n, int img_res, int grid, int bg_erosion,
                                             int32_t* pairs, int32_t* bg_lists, uint8_t* bg_masks, int32_t* counts,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  return dh_cells_from_correspondences_vacated(corr, n, img_res, grid, bg_erosion, pairs, bg_lists, bg_masks, counts, workspace,
                                               workspace_bytes, stream, nullptr);
}
