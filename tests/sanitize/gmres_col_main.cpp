// Stand-alone check of the per-column host bookkeeping of the block GMRES (csrc/gmres_col.h): built with
// -fsanitize=address,undefined and run by tests/test_gmres_col_sanitized.py.  No backend, no device: a random upper
// Hessenberg matrix per column, fed step by step as PC::solve_gmres_block feeds it, with columns that freeze in the middle
// of a cycle, a remainder of exactly 0, a cycle that starts from a zero residual and a restart.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gmres_col.h"

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
      ++fails;                                                    \
    }                                                             \
  } while (0)

// || beta e_1 - Hbar(0 .. k, 0 .. k - 1) y ||, Hbar row-major (m + 1) x m
static double ls_residual(const std::vector<double>& hb, int m, int k, double beta, const std::vector<double>& y) {
  long double s2 = 0.0L;
  for (int i = 0; i <= k; ++i) {
    long double r = i == 0 ? beta : 0.0;
    for (int j = 0; j < k; ++j) r -= (long double)hb[(size_t)i * m + j] * y[j];
    s2 += r * r;
  }
  return (double)std::sqrt(s2);
}

int main() {
  std::mt19937_64 gen(7);
  std::normal_distribution<double> nd;
  const int w = 4;                                     // columns of a slab: the dots of a step lie w apart
  for (int m : {1, 2, 7, 30}) {
    std::vector<geneo::GmresColumn> col(w);
    std::vector<std::vector<double>> hb(w, std::vector<double>((size_t)(m + 1) * m, 0.0));
    std::vector<double> beta(w), dots((size_t)(m + 1) * w);
    for (int cycle = 0; cycle < 2; ++cycle) {          // the second cycle: a restart on the same objects
      for (int j = 0; j < w; ++j) {
        if (cycle == 0) col[j].init(m);
        beta[j] = j == 3 ? 0.0 : 1.0 + std::fabs(nd(gen));       // column 3 starts from a zero residual: never stepped
        col[j].start(beta[j]);
        std::fill(hb[j].begin(), hb[j].end(), 0.0);
      }
      const int freeze_at = m / 2;                     // column 1 freezes after this many steps
      for (int k = 0; k < m; ++k) {
        for (int j = 0; j < w; ++j) {
          if (j == 3 || (j == 1 && k >= freeze_at)) continue;
          for (int i = 0; i <= k; ++i) dots[(size_t)i * w + j] = nd(gen);
          double hn = std::fabs(nd(gen)) + 0.1;
          if (j == 2 && k == m - 1) hn = 0.0;          // the Krylov space is exhausted in column 2's last step
          for (int i = 0; i <= k; ++i) hb[j][(size_t)i * m + k] = dots[(size_t)i * w + j];
          hb[j][(size_t)(k + 1) * m + k] = hn;
          const double rn = col[j].step(dots.data() + j, (size_t)w, hn);
          CHECK(col[j].k == k + 1);
          CHECK(std::isfinite(rn) && rn >= 0.0);
          geneo::GmresColumn probe = col[j];           // y of the system as it stands, without disturbing the column
          probe.solve();
          const double ref = ls_residual(hb[j], m, k + 1, beta[j], probe.y);
          CHECK(std::fabs(rn - ref) <= 1e-10 * beta[j]);
          if (hn == 0.0) CHECK(rn == 0.0);
        }
        if (k + 1 == freeze_at) {
          col[1].solve();
          for (int i = freeze_at; i < m; ++i) CHECK(col[1].y[i] == 0.0);
        }
      }
      for (int j = 0; j < w; ++j) {
        if (j != 1 || freeze_at == 0) col[j].solve();
        for (double v : col[j].y) CHECK(std::isfinite(v));
        CHECK((int)col[j].y.size() == m);
      }
      for (double v : col[3].y) CHECK(v == 0.0);       // never stepped: no contribution to the solution update
      CHECK(col[3].k == 0);
      if (freeze_at > 0) CHECK(col[1].k == freeze_at);
      const double before = col[0].g[m];
      CHECK(col[0].step(dots.data(), (size_t)w, 1.0) == std::fabs(before));    // a step past the restart writes nothing
      CHECK(col[0].k == m);
    }
  }
  std::printf(fails ? "gmres_col: %d checks failed\n" : "gmres_col: ok\n", fails);
  return fails ? 1 : 0;
}
