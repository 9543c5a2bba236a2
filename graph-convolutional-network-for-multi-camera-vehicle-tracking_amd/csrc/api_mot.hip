// C ABI of the CLEAR MOT scores (include/mtmc_mpn.h): mtmc_mot_pairs checks its arguments and enqueues the
// candidate pass of mot_metrics.hip; mtmc_mot_walk is the host half, the frame-by-frame correspondence walk of motmetrics'
// MOTAccumulator.update over the sorted candidates, with the per-object statistics.  It touches no GPU: the walk is a
// chain of dependent steps that touches each row once, the device did the part that grows with the pairs.
#include "api_error.h"
#include "assign.h"
#include "mot_metrics.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {

using mtmc_api::fail;
using mtmc_assign::LexCost;

constexpr int64_t kRowLimit = (int64_t)1 << 31;

enum { kMatches, kSwitches, kMisses, kFalsePositives, kFragmentations, kMostlyTracked, kPartiallyTracked, kMostlyLost,
       kUniqueObjects, kObjects, kPredictions, kFrames };
static_assert(kFrames + 1 == MTMC_MOT_COUNTS, "counts [MTMC_MOT_COUNTS] of mtmc_mot_walk");

struct Side {
  const int32_t* group; const int32_t* ident; const uint8_t* keep; int64_t n; int64_t n_ident;
  bool kept(int64_t i) const { return !keep || keep[i]; }
};

// rows sorted by group, and (ground truth: by identity inside a group); every value inside its range
const char* side_refused(const Side& s, int64_t n_groups, bool sorted_ident) {
  for (int64_t i = 0; i < s.n; ++i) {
    if (s.group[i] < 0 || s.group[i] >= n_groups || s.ident[i] < 0 || s.ident[i] >= s.n_ident)
      return "a row's group or identity is outside [0, n_groups) / [0, n_identities)";
    if (i > 0 && (s.group[i] < s.group[i - 1] || (sorted_ident && s.group[i] == s.group[i - 1] && s.ident[i] < s.ident[i - 1])))
      return "rows are not sorted by group (ground truth: by group, then identity)";
  }
  return nullptr;
}

struct Walk {
  const int32_t* pairs; const double* dist; int64_t n_pairs;
  Side gt, pr; const int64_t* position;
  int64_t* counts; double* dist_sum; int32_t* match_of_row; int64_t* stats;

  std::vector<int32_t> last_match;                     // m[o]: the predicted identity o was last matched to, -1: none yet
  std::vector<int64_t> hyp_group, hyp_row;             // the group in which h was last seen, and its row there
  std::vector<int64_t> rows_of, tracked_of;            // per ground-truth identity: rows, tracked rows
  std::vector<char> last_event;                        // 0: no row yet, 1: tracked, 2: a miss after a tracked row
  // one group
  std::vector<int64_t> cand_begin, mate, by_position;  // per ground-truth row of the group: its candidates, its prediction row
  std::vector<double> mate_dist;
  std::vector<char> taken, is_switch;                  // taken: per prediction row of the group
  struct Edge { int32_t r, c; double d; int32_t comp; };
  std::vector<Edge> edges;
  std::vector<int32_t> parent, deg, local, comp_of;
  std::vector<LexCost> cost;
  std::vector<int> col_of_row;
  std::vector<int32_t> comp_rows, comp_cols;

  int32_t find(int32_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  }

  void match(int64_t r_local, int64_t c_local, double d, int64_t gs, int64_t ps) {
    mate[r_local] = ps + c_local;
    mate_dist[r_local] = d;
    taken[c_local] = 1;
    const int32_t before = last_match[gt.ident[gs + r_local]];
    is_switch[r_local] = before >= 0 && before != pr.ident[ps + c_local];
  }

  // step 2 over the edges between rows not taken: the most pairs, then the smallest sum
  void assign(int64_t ng, int64_t np, int64_t gs, int64_t ps) {
    deg.assign(ng + np, 0);
    bool choice = false;
    for (const Edge& e : edges) {
      choice |= ++deg[e.r] > 1;
      choice |= ++deg[ng + e.c] > 1;
    }
    if (!choice) {                                     // no row has two candidates: every edge is a pair
      for (const Edge& e : edges) match(e.r, e.c, e.d, gs, ps);
      return;
    }
    parent.resize(ng + np);
    for (int64_t x = 0; x < ng + np; ++x) parent[x] = (int32_t)x;
    for (const Edge& e : edges) {
      const int32_t a = find(e.r), b = find((int32_t)(ng + e.c));
      if (a != b) parent[b] = a;
    }
    comp_of.assign(ng + np, -1);
    local.assign(ng + np, -1);
    comp_rows.clear(); comp_cols.clear();
    for (int64_t x = 0; x < ng + np; ++x) {            // ascending: local row / column numbers follow the rows' order
      if (!deg[x]) continue;
      const int32_t root = find((int32_t)x);
      if (comp_of[root] < 0) { comp_of[root] = (int32_t)comp_rows.size(); comp_rows.push_back(0); comp_cols.push_back(0); }
      const int32_t c = comp_of[x] = comp_of[root];
      local[x] = x < ng ? comp_rows[c]++ : comp_cols[c]++;
    }
    for (Edge& e : edges) e.comp = comp_of[e.r];
    std::stable_sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) { return a.comp < b.comp; });
    if (stats) ++stats[0];
    for (size_t q0 = 0; q0 < edges.size();) {
      size_t q1 = q0;
      while (q1 < edges.size() && edges[q1].comp == edges[q0].comp) ++q1;
      const int64_t rows = comp_rows[edges[q0].comp], cols = comp_cols[edges[q0].comp];
      if (q1 - q0 == 1) {
        match(edges[q0].r, edges[q0].c, edges[q0].d, gs, ps);
      } else {
        if (stats && (rows * cols > stats[1] * stats[2] || (rows * cols == stats[1] * stats[2] && rows > stats[1]))) {
          stats[1] = rows; stats[2] = cols;
        }
        const bool flip = rows > cols;                 // the solver wants its shorter side as rows
        const int n = (int)(flip ? cols : rows), m = (int)(flip ? rows : cols);
        LexCost forbidden;
        forbidden.big = 1;
        cost.assign((size_t)n * m, forbidden);
        for (size_t q = q0; q < q1; ++q) {
          const int32_t lr = local[edges[q].r], lc = local[ng + edges[q].c];
          LexCost& slot = flip ? cost[(size_t)lc * m + lr] : cost[(size_t)lr * m + lc];
          slot.big = 0;
          slot.d = edges[q].d;
        }
        LexCost inf;
        inf.big = INT64_MAX / 4;
        const LexCost* w = cost.data();
        mtmc_assign::assign_rows<LexCost>(n, m, [w, m](int i, int j) { return w[(size_t)i * m + j]; }, inf, col_of_row);
        for (size_t q = q0; q < q1; ++q) {
          const int32_t lr = local[edges[q].r], lc = local[ng + edges[q].c];
          if (flip ? col_of_row[lc] == lr : col_of_row[lr] == lc) match(edges[q].r, edges[q].c, edges[q].d, gs, ps);
        }
      }
      q0 = q1;
    }
  }

  int32_t run() {
    int64_t gi = 0, pi = 0, ki = 0, prev_r = -1, prev_c = -1;
    double sum = 0.0;
    while (gi < gt.n || pi < pr.n) {
      const int64_t g = gi < gt.n && (pi >= pr.n || gt.group[gi] <= pr.group[pi]) ? gt.group[gi] : pr.group[pi];
      const int64_t gs = gi, ps = pi;
      while (gi < gt.n && gt.group[gi] == g) ++gi;
      while (pi < pr.n && pr.group[pi] == g) ++pi;
      const int64_t ng = gi - gs, np = pi - ps;
      bool any = false;
      taken.assign(np, 0);
      for (int64_t c = ps; c < pi; ++c) {
        if (!pr.kept(c)) { taken[c - ps] = 2; continue; }  // (2: not there at all)
        any = true;
        const int32_t h = pr.ident[c];
        if (hyp_group[h] == g)
          return fail(MTMC_E_ARG, "mot_walk: predicted identity %d is kept twice in group %lld (rows %lld and %lld): "
                      "the walk needs drop_repeats", h, (long long)g, (long long)hyp_row[h], (long long)c);
        hyp_group[h] = g;
        hyp_row[h] = c;
      }
      // the candidates of this group, row by row
      cand_begin.assign(ng + 1, ki);
      int64_t ke = ki;
      for (; ke < n_pairs && pairs[3 * ke + 1] < gi; ++ke) {
        const int64_t pg = pairs[3 * ke], r = pairs[3 * ke + 1], c = pairs[3 * ke + 2];
        if (r < 0 || r >= gt.n || c < 0 || c >= pr.n)
          return fail(MTMC_E_ARG, "mot_walk: candidate %lld = (%lld, %lld, %lld) names a row outside [0, %lld) x [0, %lld)",
                      (long long)ke, (long long)pg, (long long)r, (long long)c, (long long)gt.n, (long long)pr.n);
        if (r < prev_r || (r == prev_r && c <= prev_c))
          return fail(MTMC_E_ARG, "mot_walk: candidate %lld is not sorted by (group, ground-truth row, prediction row), or is "
                      "listed twice", (long long)ke);
        if (r < gs || pg != g || c < ps || c >= pi || !gt.kept(r) || !pr.kept(c) || !(dist[ke] == dist[ke]))
          return fail(MTMC_E_ARG, "mot_walk: candidate %lld = (%lld, %lld, %lld) joins rows of two groups, a row that is not "
                      "kept, or has a NaN distance", (long long)ke, (long long)pg, (long long)r, (long long)c);
        prev_r = r; prev_c = c;
        cand_begin[r - gs + 1] = ke + 1;
      }
      for (int64_t r = 0; r < ng; ++r) cand_begin[r + 1] = std::max(cand_begin[r + 1], cand_begin[r]);
      mate.assign(ng, -1);
      mate_dist.assign(ng, 0.0);
      is_switch.assign(ng, 0);
      // step 1, continuity: in input order, an identity keeps the prediction it was last matched to while that is a candidate
      by_position.clear();
      for (int64_t r = gs; r < gi; ++r)
        if (gt.kept(r)) { any = true; if (last_match[gt.ident[r]] >= 0) by_position.push_back(r); }
      const auto earlier = [this](int64_t a, int64_t b) { return position[a] < position[b]; };
      if (!std::is_sorted(by_position.begin(), by_position.end(), earlier))     // (a table sorted by id within a frame is)
        std::sort(by_position.begin(), by_position.end(), earlier);
      for (const int64_t r : by_position) {
        const int32_t h = last_match[gt.ident[r]];
        if (hyp_group[h] != g || taken[hyp_row[h] - ps]) continue;
        for (int64_t k = cand_begin[r - gs]; k < cand_begin[r - gs + 1]; ++k)
          if (pairs[3 * k + 2] == hyp_row[h]) {
            mate[r - gs] = hyp_row[h];
            mate_dist[r - gs] = dist[k];
            taken[hyp_row[h] - ps] = 1;
            break;
          }
      }
      // step 2, assignment over the rows not taken
      edges.clear();
      for (int64_t k = ki; k < ke; ++k) {
        const int64_t r = pairs[3 * k + 1] - gs, c = pairs[3 * k + 2] - ps;
        if (mate[r] < 0 && !taken[c]) edges.push_back({(int32_t)r, (int32_t)c, dist[k], 0});
      }
      if (!edges.empty()) assign(ng, np, gs, ps);
      ki = ke;
      // steps 3 and 4 and the statistics, in the order of the ground-truth identities
      for (int64_t r = gs; r < gi; ++r) {
        if (!gt.kept(r)) { match_of_row[r] = -2; continue; }
        const int32_t o = gt.ident[r];
        ++counts[kObjects];
        if (rows_of[o]++ == 0) ++counts[kUniqueObjects];
        match_of_row[r] = (int32_t)mate[r - gs];
        if (mate[r - gs] >= 0) {
          ++counts[is_switch[r - gs] ? kSwitches : kMatches];
          sum += mate_dist[r - gs];
          last_match[o] = pr.ident[mate[r - gs]];
          ++tracked_of[o];
          if (last_event[o] == 2) ++counts[kFragmentations];   // tracked again after a miss that followed a tracked row
          last_event[o] = 1;
        } else {
          ++counts[kMisses];
          if (last_event[o] == 1) last_event[o] = 2;
        }
      }
      for (int64_t c = 0; c < np; ++c) {
        if (taken[c] != 2) ++counts[kPredictions];
        if (taken[c] == 0) ++counts[kFalsePositives];
      }
      if (any) ++counts[kFrames];
    }
    if (ki < n_pairs) {                                  // a ground-truth row at or past the last one
      if (pairs[3 * ki + 1] >= gt.n)
        return fail(MTMC_E_ARG, "mot_walk: candidate %lld = (%d, %d, %d) names a row outside [0, %lld) x [0, %lld)", (long long)ki,
                    pairs[3 * ki], pairs[3 * ki + 1], pairs[3 * ki + 2], (long long)gt.n, (long long)pr.n);
      return fail(MTMC_E_ARG, "mot_walk: candidate %lld is not sorted by (group, ground-truth row, prediction row), or is "
                  "listed twice", (long long)ki);
    }
    for (int64_t o = 0; o < gt.n_ident; ++o) {
      if (!rows_of[o]) continue;
      const int64_t t = tracked_of[o], n = rows_of[o];
      ++counts[5 * t >= 4 * n ? kMostlyTracked : (5 * t < n ? kMostlyLost : kPartiallyTracked)];
    }
    *dist_sum = sum;
    return MTMC_OK;
  }
};

const char* mot_sizes_refused(int64_t n_gt, int64_t n_pred, int64_t n_groups) {
  if (n_gt < 0 || n_pred < 0 || n_groups < 0 || n_gt >= kRowLimit || n_pred >= kRowLimit || n_groups >= kRowLimit)
    return "n_gt, n_pred and n_groups must be in [0, 2^31)";
  return nullptr;
}

}  // namespace

extern "C" {

size_t mtmc_mot_pairs_workspace_bytes(int64_t n_groups) {
  return mot_sizes_refused(0, 0, n_groups) ? 0 : mtmc::mot_layout(n_groups).total;
}

int32_t mtmc_mot_pairs(const double* gt_boxes, const int64_t* gt_offsets, const uint8_t* gt_keep, int64_t n_gt,
                       const double* pred_boxes, const int64_t* pred_offsets, const uint8_t* pred_keep, int64_t n_pred,
                       int64_t n_groups, double max_dist, int32_t* pairs, double* dist, int64_t max_pairs, int64_t* n_pairs,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (const char* why = mot_sizes_refused(n_gt, n_pred, n_groups)) return fail(MTMC_E_ARG, "mot_pairs: %s", why);
  if (!n_pairs || max_pairs < 0 || (max_pairs > 0 && (!pairs || !dist)))
    return fail(MTMC_E_ARG, "mot_pairs: NULL n_pairs, pairs or dist, or max_pairs < 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool any = n_gt > 0 && n_pred > 0 && n_groups > 0;
  if (any && (!gt_boxes || !gt_offsets || !pred_boxes || !pred_offsets || !pred_keep || !workspace || ((uintptr_t)workspace & 7)))
    return fail(MTMC_E_ARG, "mot_pairs: NULL boxes, offsets or pred_keep, or a NULL or misaligned workspace");
  const mtmc::MotLayout lo = mtmc::mot_layout(n_groups);
  if (any && workspace_bytes < lo.total)
    return fail(MTMC_E_ARG, "mot_pairs: workspace has %zu bytes, %zu needed (mtmc_mot_pairs_workspace_bytes)", workspace_bytes,
                lo.total);
  if (hipMemsetAsync(n_pairs, 0, sizeof(int64_t), s) != hipSuccess) return fail(MTMC_E_HIP, "mot_pairs: hipMemsetAsync failed");
  if (!any) return MTMC_OK;
  mtmc::MotPairsArgs a;
  a.side.gt_boxes = gt_boxes; a.side.pr_boxes = pred_boxes; a.side.gt_off = gt_offsets; a.side.pr_off = pred_offsets;
  a.side.gt_ident = nullptr; a.side.pr_ident = nullptr; a.side.gt_keep = gt_keep; a.side.pr_keep = pred_keep;
  a.side.n_gt = n_gt; a.side.n_pr = n_pred; a.side.n_groups = n_groups; a.side.n_obj = 0; a.side.n_hyp = 0;
  a.side.max_dist = max_dist;
  a.side.prefix = reinterpret_cast<long long*>(static_cast<char*>(workspace) + lo.prefix);
  a.side.cells = nullptr;
  a.pairs = pairs; a.dist = dist; a.max_pairs = max_pairs;
  a.counter = reinterpret_cast<unsigned long long*>(n_pairs);
  mtmc::launch_mot_pairs(a, s);
  return mtmc_api::launched("mot_pairs");
}

int32_t mtmc_mot_walk(const int32_t* pairs, const double* dist, int64_t n_pairs, const int32_t* gt_group,
                      const int32_t* gt_identity, const int64_t* gt_position, const uint8_t* gt_keep, int64_t n_gt,
                      const int32_t* pred_group, const int32_t* pred_identity, const uint8_t* pred_keep, int64_t n_pred,
                      int64_t n_groups, int64_t n_obj, int64_t n_hyp, int64_t* counts, double* dist_sum, int32_t* match_of_row,
                      int64_t* stats) {
  if (const char* why = mot_sizes_refused(n_gt, n_pred, n_groups)) return fail(MTMC_E_ARG, "mot_walk: %s", why);
  if (n_pairs < 0 || n_obj < 0 || n_hyp < 0 || n_obj > n_gt || n_hyp > n_pred)
    return fail(MTMC_E_ARG, "mot_walk: n_pairs must be >= 0, n_obj in [0, n_gt] and n_hyp in [0, n_pred]");
  if (!counts || !dist_sum || (n_pairs > 0 && (!pairs || !dist)) ||
      (n_gt > 0 && (!gt_group || !gt_identity || !gt_position || !match_of_row)) || (n_pred > 0 && (!pred_group || !pred_identity)))
    return fail(MTMC_E_ARG, "mot_walk: NULL pairs, dist, group, identity, position, counts, dist_sum or match_of_row");
  for (int k = 0; k < MTMC_MOT_COUNTS; ++k) counts[k] = 0;
  *dist_sum = 0.0;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  const Side gt{gt_group, gt_identity, gt_keep, n_gt, n_obj}, pr{pred_group, pred_identity, pred_keep, n_pred, n_hyp};
  if (const char* why = side_refused(gt, n_groups, true)) return fail(MTMC_E_ARG, "mot_walk: ground truth: %s", why);
  if (const char* why = side_refused(pr, n_groups, false)) return fail(MTMC_E_ARG, "mot_walk: predictions: %s", why);
  try {
    Walk w;
    w.pairs = pairs; w.dist = dist; w.n_pairs = n_pairs; w.gt = gt; w.pr = pr; w.position = gt_position;
    w.counts = counts; w.dist_sum = dist_sum; w.match_of_row = match_of_row; w.stats = stats;
    w.last_match.assign(n_obj, -1);
    w.hyp_group.assign(n_hyp, -1);
    w.hyp_row.assign(n_hyp, -1);
    w.rows_of.assign(n_obj, 0);
    w.tracked_of.assign(n_obj, 0);
    w.last_event.assign(n_obj, 0);
    return w.run();
  } catch (const std::bad_alloc&) {
    return fail(MTMC_E_ARG, "mot_walk: out of host memory");
  }
}

}  // extern "C"
