// Stand-alone check of the window bookkeeping of the flexible CG (csrc/fcg_window.h): built with
// -fsanitize=address,undefined and run by tests/test_fcg_window_sanitized.py.  No backend, no device: for mmax in
// {1, 2, 5, 30} and both truncation types, every iteration i up to 3 (mmax + 1) against a brute-force list of the
// directions alive -- the window is the m_i most recent ones, contiguous in a doubled table that is indexed as the driver
// indexes it, the slot of the new direction is none of the window's, and the eta ring still holds every window member's.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "fcg_window.h"

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
      ++fails;                                                    \
    }                                                             \
  } while (0)

int main() {
  for (int mmax : {1, 2, 5, 30}) {
    for (int notay = 0; notay < 2; ++notay) {
      geneo::FcgWindow win;
      win.init(mmax, notay != 0);
      CHECK(win.slots == mmax + 1 && win.table_entries() == 2 * (mmax + 1));
      CHECK((int)win.eta.size() == win.slots);
      // the doubled table as the driver fills it: entry j and entry j + slots name slot j; here the direction in the slot
      std::vector<int> table((size_t)win.table_entries(), -1);
      std::vector<int> alive;                          // brute force: every direction made so far, oldest first
      int largest = 0;
      for (int i = 0; i <= 3 * (mmax + 1); ++i) {
        const int m = win.size(i);
        const int mi = notay ? std::max(1, i % (mmax + 1)) : mmax;
        CHECK(m == std::min(i, mi) && m >= 0 && m <= mmax && m <= (int)alive.size());
        CHECK(i == 0 || m >= 1);
        CHECK(win.first(i) == i - m);
        const int off = win.offset(i);
        CHECK(off >= 0 && off + m <= win.table_entries());
        for (int j = 0; j < m; ++j) {                  // the window: the m most recent directions, oldest first
          const int want = alive[alive.size() - (size_t)m + (size_t)j];
          CHECK(want == i - m + j);
          CHECK(table[(size_t)(off + j)] == want);
          CHECK(win.eta_of(want) == 1.0 + want);       // not yet overwritten by a later direction
          CHECK(win.slot(want) != win.slot(i));        // z is written into a slot no window member lives in
        }
        largest = std::max(largest, m);
        CHECK(win.max_size(i + 1) == largest);
        // direction i is made: its slot, both table entries, its eta
        const int s = win.slot(i);
        CHECK(s >= 0 && s < win.slots);
        table[(size_t)s] = table[(size_t)(s + win.slots)] = i;
        win.eta_of(i) = 1.0 + i;
        alive.push_back(i);
      }
      CHECK(win.max_size(0) == 0);
      CHECK(largest == mmax);
    }
  }
  std::printf(fails ? "fcg_window: %d checks failed\n" : "fcg_window: ok\n", fails);
  return fails ? 1 : 0;
}
