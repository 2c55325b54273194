// Host bookkeeping of the truncation window of the flexible CG (PC::solve_fcg): which ring slot direction i lives in, how
// many of the directions before it iteration i orthogonalises against, where that window starts in a pointer table that
// names every slot twice, and eta_k = (A p_k, p_k) of the directions a window can still reach.
// Header-only and free of the backend: a stand-alone program runs it under a sanitizer (tests/sanitize/fcg_window_main.cpp).
//
// Iteration i makes p_i from z_i and the m_i = min(i, mi) most recent directions p_{i - m_i} .. p_{i - 1};
//   notay:    mi = max(1, i mod (mmax + 1))     the window grows from 1 to mmax and starts again (Notay's FCG(mmax))
//   standard: mi = mmax                         the mmax most recent directions, always
// m_i <= mmax either way, and p_i is written while all of them are still read: the ring has mmax + 1 slots, direction i in
// slot i mod (mmax + 1) (PETSc's KSPFCG holds mmax + 1 directions for the same reason).  In a table of 2 (mmax + 1)
// entries whose entries j and j + mmax + 1 name the vector of slot j, the window of iteration i is the m_i consecutive
// entries from offset(i) on, oldest first.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace geneo {

struct FcgWindow {
  int mmax = 1, slots = 2;
  bool notay = true;
  std::vector<double> eta;           // eta of the direction in every ring slot

  void init(int mmax_, bool notay_) {
    mmax = std::max(1, mmax_);
    slots = mmax + 1;
    notay = notay_;
    eta.assign((size_t)slots, 0.0);
  }
  int table_entries() const { return 2 * slots; }
  int slot(int i) const { return i % slots; }
  int size(int i) const {
    const int mi = notay ? std::max(1, i % (mmax + 1)) : mmax;
    return std::min(i, mi);
  }
  int first(int i) const { return i - size(i); }                 // the oldest direction of the window of iteration i
  int offset(int i) const { return first(i) % slots; }           // its entry in the doubled table; offset + size <= 2 mmax
  double& eta_of(int k) { return eta[(size_t)(k % slots)]; }     // direction k, while a window can reach it
  int max_size(int its) const {                                  // the largest window of iterations 0 .. its - 1
    int m = 0;
    for (int i = 0; i < its && m < mmax; ++i) m = std::max(m, size(i));
    return m;
  }
};

}  // namespace geneo
