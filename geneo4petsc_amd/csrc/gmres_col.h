// Host bookkeeping of ONE column of the block GMRES (PC::solve_gmres_block): its Hessenberg matrix, Givens rotations,
// rotated right-hand side and, once the column is frozen or its cycle ends, the coefficients y of its solution update.
// Statement for statement the arithmetic of PC::solve_gmres, so that a column of a block counts the iterations its
// single-vector solve counts.  Header-only and free of the backend: a stand-alone program can run it under a sanitizer
// (tests/sanitize/gmres_col_main.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace geneo {

struct GmresColumn {
  int m = 0;                         // restart length
  int k = 0;                         // steps of the current cycle that entered this column's system
  std::vector<double> h, cs, sn, g, y;

  void init(int restart) {
    m = std::max(1, restart);
    h.assign((size_t)(m + 1) * m, 0.0);
    cs.assign(m, 0.0);
    sn.assign(m, 0.0);
    g.assign(m + 1, 0.0);
    y.assign(m, 0.0);
    k = 0;
  }
  // a cycle starts from a residual of norm rn; y = 0 until solve() (a column frozen in an earlier cycle keeps y = 0)
  void start(double rn) {
    std::fill(g.begin(), g.end(), 0.0);
    std::fill(y.begin(), y.end(), 0.0);
    g[0] = rn;
    k = 0;
  }
  // Step k of the cycle: dots[i * stride] = (v_i, w), i <= k, and hn = |w - sum_i dots_i v_i|.  Returns the residual norm.
  double step(const double* dots, size_t stride, double hn) {
    if (k >= m) return std::fabs(g[m]);
    for (int j = 0; j <= k; ++j) h[(size_t)j * m + k] = dots[(size_t)j * stride];
    h[(size_t)(k + 1) * m + k] = hn;
    for (int j = 0; j < k; ++j) {
      const double a = h[(size_t)j * m + k], c = h[(size_t)(j + 1) * m + k];
      h[(size_t)j * m + k] = cs[j] * a + sn[j] * c;
      h[(size_t)(j + 1) * m + k] = -sn[j] * a + cs[j] * c;
    }
    const double den = std::hypot(h[(size_t)k * m + k], h[(size_t)(k + 1) * m + k]);
    cs[k] = h[(size_t)k * m + k] / den;
    sn[k] = h[(size_t)(k + 1) * m + k] / den;
    h[(size_t)k * m + k] = den;
    h[(size_t)(k + 1) * m + k] = 0.0;
    g[k + 1] = -sn[k] * g[k];
    g[k] = cs[k] * g[k];
    ++k;
    return std::fabs(g[k]);
  }
  // y of the k x k triangular system; rows i >= k stay zero
  void solve() {
    for (int i = k - 1; i >= 0; --i) {
      double s = g[i];
      for (int j = i + 1; j < k; ++j) s -= h[(size_t)i * m + j] * y[j];
      y[i] = s / h[(size_t)i * m + i];
    }
    for (int i = k; i < m; ++i) y[i] = 0.0;
  }
};

}  // namespace geneo
