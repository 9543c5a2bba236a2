// C ABI of the ID scores (include/mtmc_mpn.h): mtmc_id_filter, mtmc_id_overlap and mtmc_id_cells check
// their arguments and enqueue the kernels of id_metrics.hip; mtmc_id_assign is the host half, the exact assignment that
// turns the overlap counts C into IDTP.  It touches no GPU.
#include "api_error.h"
#include "assign.h"
#include "id_metrics.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {

using mtmc_api::fail;

constexpr int64_t kRowLimit = (int64_t)1 << 31;

// Max-weight assignment of an n x m matrix of weights >= 0 (row-major, n <= m): every row gets a column, by the shared
// solver (assign.h) on the costs -w, integers throughout.  col_of_row[i] = the column of row i.  Returns the optimum.
int64_t assign_dense(const int32_t* w, int n, int m, std::vector<int>& col_of_row) {
  mtmc_assign::assign_rows<int64_t>(n, m, [w, m](int i, int j) { return -(int64_t)w[(size_t)i * m + j]; }, INT64_MAX / 4,
                                    col_of_row);
  int64_t best = 0;
  for (int i = 0; i < n; ++i)
    if (col_of_row[i] >= 0) best += w[(size_t)i * m + col_of_row[i]];
  return best;
}

int32_t find_root(std::vector<int32_t>& parent, int32_t x) {
  while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
  return x;
}

int32_t assign_components(const int32_t* cells, int64_t n_cells, int64_t n_obj, int64_t n_hyp, int64_t* idtp,
                          int32_t* match_of_obj, int64_t* stats) {
  const int64_t n_nodes = n_obj + n_hyp;
  std::vector<int32_t> parent(n_nodes);
  for (int64_t i = 0; i < n_nodes; ++i) parent[i] = (int32_t)i;
  for (int64_t k = 0; k < n_cells; ++k) {
    const int32_t o = cells[3 * k], h = cells[3 * k + 1], c = cells[3 * k + 2];
    if (o < 0 || o >= n_obj || h < 0 || h >= n_hyp || c < 0)
      return fail(MTMC_E_ARG, "id_assign: cell %lld = (%d, %d, %d) is outside [0, %lld) x [0, %lld) or negative", (long long)k,
                  o, h, c, (long long)n_obj, (long long)n_hyp);
    if (c == 0) continue;
    const int32_t a = find_root(parent, o), b = find_root(parent, (int32_t)(n_obj + h));
    if (a != b) parent[b] = a;
  }
  // components of the support graph: only identities with a non-zero cell belong to one
  std::vector<int32_t> comp_of(n_nodes, -1), comp_rows, comp_cols, local(n_nodes, -1);
  std::vector<int64_t> comp_cells;
  std::vector<char> touched(n_nodes, 0);
  for (int64_t k = 0; k < n_cells; ++k)
    if (cells[3 * k + 2] > 0) touched[cells[3 * k]] = touched[n_obj + cells[3 * k + 1]] = 1;
  for (int64_t x = 0; x < n_nodes; ++x) {              // ascending: local row / column numbers follow the identities' order
    if (!touched[x]) continue;
    const int32_t root = find_root(parent, (int32_t)x);
    if (comp_of[root] < 0) {
      comp_of[root] = (int32_t)comp_rows.size();
      comp_rows.push_back(0); comp_cols.push_back(0); comp_cells.push_back(0);
    }
    const int32_t c = comp_of[x] = comp_of[root];
    local[x] = x < n_obj ? comp_rows[c]++ : comp_cols[c]++;
  }
  const int64_t n_comp = (int64_t)comp_rows.size();
  // the cells, component by component
  std::vector<int64_t> start(n_comp + 1, 0);
  for (int64_t k = 0; k < n_cells; ++k)
    if (cells[3 * k + 2] > 0) ++start[comp_of[cells[3 * k]] + 1];
  for (int64_t c = 0; c < n_comp; ++c) start[c + 1] += start[c];
  std::vector<int64_t> order(start[n_comp]), fill(start.begin(), start.end() - 1);
  for (int64_t k = 0; k < n_cells; ++k)
    if (cells[3 * k + 2] > 0) order[fill[comp_of[cells[3 * k]]]++] = k;

  int64_t total = 0, big_rows = 0, big_cols = 0;
  std::vector<int32_t> w, obj_of_local, hyp_of_local;
  std::vector<int> col_of_row;
  for (int64_t c = 0; c < n_comp; ++c) {
    const int64_t rows = comp_rows[c], cols = comp_cols[c];
    if (rows * cols > big_rows * big_cols || (rows * cols == big_rows * big_cols && rows > big_rows)) { big_rows = rows; big_cols = cols; }
    const bool flip = rows > cols;                       // the solver wants its shorter side as rows
    const int n = (int)(flip ? cols : rows), m = (int)(flip ? rows : cols);
    w.assign((size_t)n * m, 0);
    obj_of_local.assign(rows, -1);
    hyp_of_local.assign(cols, -1);
    for (int64_t q = start[c]; q < start[c + 1]; ++q) {
      const int32_t o = cells[3 * order[q]], h = cells[3 * order[q] + 1];
      const int32_t lr = local[o], lc = local[n_obj + h];
      obj_of_local[lr] = o; hyp_of_local[lc] = h;
      int32_t& slot = flip ? w[(size_t)lc * m + lr] : w[(size_t)lr * m + lc];
      if (slot != 0) return fail(MTMC_E_ARG, "id_assign: the cell (%d, %d) is listed twice", o, h);
      slot = cells[3 * order[q] + 2];
    }
    total += assign_dense(w.data(), n, m, col_of_row);
    for (int i = 0; i < n; ++i) {
      const int j = col_of_row[i];
      if (j < 0 || w[(size_t)i * m + j] == 0) continue; // a zero-weight pairing is no match
      if (flip) match_of_obj[obj_of_local[j]] = hyp_of_local[i];
      else match_of_obj[obj_of_local[i]] = hyp_of_local[j];
    }
  }
  *idtp = total;
  if (stats) { stats[0] = n_comp; stats[1] = big_rows; stats[2] = big_cols; }
  return MTMC_OK;
}

}  // namespace

extern "C" {

int32_t mtmc_id_filter(const double* boxes, const int32_t* camera, const int32_t* identity, const int32_t* group, int64_t n_rows,
                       int64_t n_identities, int32_t n_cameras, int32_t border, double x_lo, double x_hi, double y_lo,
                       double y_hi, const uint8_t* roi, const int32_t* plane_of_camera, int32_t n_planes, int32_t roi_height,
                       int32_t roi_width, int32_t min_cameras, int32_t drop_repeats, uint8_t* stage, uint8_t* keep,
                       uint64_t* cameras, int64_t* n_kept, void* stream) {
  if (n_rows < 0 || n_rows >= kRowLimit || n_identities < 0 || n_identities > n_rows)
    return fail(MTMC_E_ARG, "id_filter: n_rows must be in [0, 2^31) and n_identities in [0, n_rows]");
  if (n_cameras < 0 || n_cameras > MTMC_ID_MAX_CAMERAS)
    return fail(MTMC_E_ARG, "id_filter: %d cameras, at most %d (one bit each in a 64-bit word)", n_cameras, MTMC_ID_MAX_CAMERAS);
  if (!n_kept || (n_rows > 0 && (!boxes || !camera || !identity || !group || !stage || !keep || !cameras)))
    return fail(MTMC_E_ARG, "id_filter: NULL boxes, camera, identity, group, stage, keep, cameras or n_kept");
  if (roi && (!plane_of_camera || n_planes < 1 || roi_height < 1 || roi_width < 1))
    return fail(MTMC_E_ARG, "id_filter: a roi needs plane_of_camera, n_planes >= 1 and a mask of at least 1 x 1");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(n_kept, 0, sizeof(int64_t), s) != hipSuccess) return fail(MTMC_E_HIP, "id_filter: hipMemsetAsync failed");
  if (n_rows == 0) return MTMC_OK;
  if (hipMemsetAsync(cameras, 0, (size_t)n_identities * sizeof(uint64_t), s) != hipSuccess)
    return fail(MTMC_E_HIP, "id_filter: hipMemsetAsync failed");
  mtmc::IdFilterArgs a;
  a.boxes = boxes; a.cam = camera; a.ident = identity; a.group = group; a.n = n_rows;
  a.n_ident = n_identities; a.n_cameras = n_cameras;
  a.x_lo = x_lo; a.x_hi = x_hi; a.y_lo = y_lo; a.y_hi = y_hi; a.border = border;
  a.roi = roi; a.plane_of_cam = plane_of_camera; a.n_planes = n_planes; a.roi_h = roi_height; a.roi_w = roi_width;
  a.min_cameras = min_cameras; a.drop_repeats = drop_repeats;
  a.stage = stage; a.keep = keep;
  a.cameras = reinterpret_cast<unsigned long long*>(cameras);
  a.kept = reinterpret_cast<unsigned long long*>(n_kept);
  mtmc::launch_id_filter(a, s);
  return mtmc_api::launched("id_filter");
}

static const char* id_sizes_refused(int64_t n_obj, int64_t n_hyp, int64_t n_groups) {
  if (n_obj < 0 || n_hyp < 0 || n_groups < 0 || n_obj >= kRowLimit || n_hyp >= kRowLimit || n_groups >= 2 * kRowLimit)
    return "n_obj, n_hyp and n_groups must be >= 0 and below 2^31 (n_groups: 2^32)";
  if (n_obj * n_hyp > MTMC_ID_MAX_CELLS) return "n_obj * n_hyp is above MTMC_ID_MAX_CELLS = 2^26 (the overlap counts are a dense table)";
  return nullptr;
}

size_t mtmc_id_overlap_workspace_bytes(int64_t n_obj, int64_t n_hyp, int64_t n_groups) {
  return id_sizes_refused(n_obj, n_hyp, n_groups) ? 0 : mtmc::id_layout(n_obj, n_hyp, n_groups).total;
}

int32_t mtmc_id_overlap(const double* gt_boxes, const int64_t* gt_offsets, const int32_t* gt_identity, const uint8_t* gt_keep,
                        int64_t n_gt, const double* pred_boxes, const int64_t* pred_offsets, const int32_t* pred_identity,
                        const uint8_t* pred_keep, int64_t n_pred, int64_t n_groups, int64_t n_obj, int64_t n_hyp,
                        double max_dist, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_gt < 0 || n_pred < 0 || n_gt >= kRowLimit || n_pred >= kRowLimit)
    return fail(MTMC_E_ARG, "id_overlap: n_gt and n_pred must be in [0, 2^31)");
  if (const char* why = id_sizes_refused(n_obj, n_hyp, n_groups)) return fail(MTMC_E_ARG, "id_overlap: %s", why);
  const bool pairs = n_gt > 0 && n_pred > 0 && n_groups > 0 && n_obj > 0 && n_hyp > 0;
  if (!workspace || ((uintptr_t)workspace & 7) ||
      (pairs && (!gt_boxes || !gt_offsets || !gt_identity || !pred_boxes || !pred_offsets || !pred_identity || !pred_keep)))
    return fail(MTMC_E_ARG, "id_overlap: NULL boxes, offsets, identity or pred_keep, or a NULL or misaligned workspace");
  const mtmc::IdLayout lo = mtmc::id_layout(n_obj, n_hyp, n_groups);
  if (workspace_bytes < lo.total)
    return fail(MTMC_E_ARG, "id_overlap: workspace has %zu bytes, %zu needed (mtmc_id_overlap_workspace_bytes)", workspace_bytes,
                lo.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  if (n_obj * n_hyp > 0 && hipMemsetAsync(ws + lo.cells, 0, (size_t)(n_obj * n_hyp) * 4, s) != hipSuccess)
    return fail(MTMC_E_HIP, "id_overlap: hipMemsetAsync failed");
  if (!pairs) return MTMC_OK;
  mtmc::IdOverlapArgs a;
  a.gt_boxes = gt_boxes; a.pr_boxes = pred_boxes; a.gt_off = gt_offsets; a.pr_off = pred_offsets;
  a.gt_ident = gt_identity; a.pr_ident = pred_identity; a.gt_keep = gt_keep; a.pr_keep = pred_keep;
  a.n_gt = n_gt; a.n_pr = n_pred; a.n_groups = n_groups; a.n_obj = n_obj; a.n_hyp = n_hyp;
  a.max_dist = max_dist;
  a.prefix = reinterpret_cast<long long*>(ws + lo.prefix);
  a.cells = reinterpret_cast<int32_t*>(ws + lo.cells);
  mtmc::launch_id_overlap(a, s);
  return mtmc_api::launched("id_overlap");
}

int32_t mtmc_id_cells(const void* workspace, int64_t n_obj, int64_t n_hyp, int32_t* cells, int64_t max_cells, int64_t* n_cells,
                      void* stream) {
  if (const char* why = id_sizes_refused(n_obj, n_hyp, 0)) return fail(MTMC_E_ARG, "id_cells: %s", why);
  if (!workspace || !n_cells || max_cells < 0 || (max_cells > 0 && !cells))
    return fail(MTMC_E_ARG, "id_cells: NULL workspace, n_cells or cells, or max_cells < 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(n_cells, 0, sizeof(int64_t), s) != hipSuccess) return fail(MTMC_E_HIP, "id_cells: hipMemsetAsync failed");
  if (n_obj * n_hyp == 0) return MTMC_OK;
  mtmc::launch_id_compact(static_cast<const int32_t*>(workspace), n_obj, n_hyp, cells, max_cells,
                          reinterpret_cast<unsigned long long*>(n_cells), s);
  return mtmc_api::launched("id_cells");
}

int32_t mtmc_id_assign(const int32_t* cells, int64_t n_cells, int64_t n_obj, int64_t n_hyp, int64_t* idtp, int32_t* match_of_obj,
                       int64_t* stats) {
  if (n_cells < 0 || n_obj < 0 || n_hyp < 0 || n_obj >= kRowLimit || n_hyp >= kRowLimit)
    return fail(MTMC_E_ARG, "id_assign: n_cells, n_obj and n_hyp must be >= 0 (the last two below 2^31)");
  if (n_obj * n_hyp > MTMC_ID_MAX_CELLS)
    return fail(MTMC_E_ARG, "id_assign: n_obj * n_hyp is above MTMC_ID_MAX_CELLS = 2^26");
  if (n_cells > n_obj * n_hyp) return fail(MTMC_E_ARG, "id_assign: more cells than n_obj * n_hyp");
  if (!idtp || (n_cells > 0 && !cells) || (n_obj > 0 && !match_of_obj))
    return fail(MTMC_E_ARG, "id_assign: NULL cells, idtp or match_of_obj");
  for (int64_t o = 0; o < n_obj; ++o) match_of_obj[o] = -1;
  *idtp = 0;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  try {
    return assign_components(cells, n_cells, n_obj, n_hyp, idtp, match_of_obj, stats);
  } catch (const std::bad_alloc&) {
    return fail(MTMC_E_ARG, "id_assign: out of host memory");
  }
}

}  // extern "C"
