// The exact assignment shared by the two host-only entries: mtmc_id_assign (api_id.hip: integer overlap counts) and
// mtmc_mot_walk (api_mot.hip: fp64 distances with forbidden pairs).  Shortest augmenting paths with potentials, the
// Hungarian method in its O(n^2 m) form, over any cost type that is an ordered group under + and -: int64_t, or the
// lexicographic pair of LexCost.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mtmc_assign {

// Minimum-cost assignment of n rows to m >= n columns: every row gets a column.  cost(i, j) is read O(n m) times per
// row; `inf` is above every sum of n costs.  col_of_row[i] = the column of row i.
template <class T, class Cost>
void assign_rows(int n, int m, Cost&& cost, const T inf, std::vector<int>& col_of_row) {
  std::vector<T> u(n + 1, T()), v(m + 1, T()), minv(m + 1);
  std::vector<int> p(m + 1, 0), way(m + 1, 0);
  std::vector<char> used(m + 1);
  for (int i = 1; i <= n; ++i) {
    p[0] = i;
    int j0 = 0;
    std::fill(minv.begin(), minv.end(), inf);
    std::fill(used.begin(), used.end(), 0);
    do {
      used[j0] = 1;
      const int i0 = p[j0];
      T delta = inf;
      int j1 = 0;
      for (int j = 1; j <= m; ++j) {
        if (used[j]) continue;
        const T cur = cost(i0 - 1, j - 1) - u[i0] - v[j];
        if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
        if (minv[j] < delta) { delta = minv[j]; j1 = j; }
      }
      for (int j = 0; j <= m; ++j) {
        if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
        else minv[j] -= delta;
      }
      j0 = j1;
    } while (p[j0] != 0);
    do {
      const int j1 = way[j0];
      p[j0] = p[j1];
      j0 = j1;
    } while (j0);
  }
  col_of_row.assign(n, -1);
  for (int j = 1; j <= m; ++j)
    if (p[j]) col_of_row[p[j] - 1] = j - 1;
}

// (forbidden pairs used, sum of distances), compared in that order: the smallest assignment has the most permitted pairs
// and among those the smallest sum.  No big constant is added to a distance, so none of its bits is lost to one.
struct LexCost {
  int64_t big = 0;
  double d = 0.0;
  LexCost operator+(const LexCost& o) const { return {big + o.big, d + o.d}; }
  LexCost operator-(const LexCost& o) const { return {big - o.big, d - o.d}; }
  LexCost& operator+=(const LexCost& o) { big += o.big; d += o.d; return *this; }
  LexCost& operator-=(const LexCost& o) { big -= o.big; d -= o.d; return *this; }
  bool operator<(const LexCost& o) const { return big < o.big || (big == o.big && d < o.d); }
};

}  // namespace mtmc_assign
