// test_lattice.cpp -- the cell index of the pair and two-profile sweeps (machineboss_amd/csrc/mb_profile_lattice.h) against a
// brute-force membership set, on the host: RectCells over a few rectangles, EnvCells over every envelope env_add accepts for
// I, L <= 4 and over bands whose i passes 64 (and, at (70, 70), whose M does).  Prints "LATTICE OK" and the tallies; any failed check
// prints its place and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "mb_profile_lattice.h"

using namespace mb;
typedef std::set<std::pair<int, int>> Members;      // (r, i): ordered row by row, ascending i

// the case at hand, for the report of a failed check
static std::string g_case;
static int g_I = 0, g_L = 0;
static const std::vector<int32_t> *g_st = nullptr, *g_en = nullptr;
static void failed(const char *file, int line, const char *cond) {
  std::printf("FAILED %s:%d: %s   [%s I=%d L=%d", file, line, cond, g_case.c_str(), g_I, g_L);
  for (size_t r = 0; g_st && r < g_st->size(); ++r) std::printf(" %d:%d", (int)(*g_st)[r], (int)(*g_en)[r]);
  std::printf("]\n");
  std::exit(1);
}
#define CHECK(cond) do { if (!(cond)) failed(__FILE__, __LINE__, #cond); } while (0)

// (a) .. (e) of one lattice.  rowMajor: index counts row by row (an envelope), else input position by input position (the rectangle).
// bounded: inside() answers for neighbours one step outside too.  columns: AXIS 1 may be asked.
template <class Cells>
static void check(const Cells &c, int I, int L, const Members &mem, bool rowMajor, bool bounded, bool columns) {
  // (a) the diagonal runs partition the member cells
  Members seen;
  std::vector<std::vector<std::pair<int, int>>> byDiag((size_t)(I + L + 1));
  for (int d = 0; d <= I + L; ++d) {
    int ilo = -7, n = -7;
    c.diag(d, ilo, n);
    CHECK(n >= 0 && n <= c.M);
    for (int i = ilo; i < ilo + n; ++i) {
      CHECK(mem.count({d - i, i}) && seen.insert({d - i, i}).second);
      byDiag[(size_t)d].push_back({d - i, i});
    }
  }
  CHECK(seen == mem);
  // (b) inside is membership
  for (int r = bounded ? -1 : 0; r <= (bounded ? L + 1 : L); ++r)
    for (int i = bounded ? -1 : 0; i <= (bounded ? I + 1 : I); ++i) CHECK(c.inside(i, r) == (mem.count({r, i}) != 0));
  // (c) index is a bijection onto 0 .. cells() - 1 in the lattice's order, cell its inverse
  CHECK(c.cells() == (long long)mem.size());
  std::vector<std::pair<int, int>> order(mem.begin(), mem.end());      // row by row
  if (!rowMajor) {
    order.clear();
    for (int i = 0; i <= I; ++i)
      for (int r = 0; r <= L; ++r) order.push_back({r, i});
  }
  for (size_t n = 0; n < order.size(); ++n) {
    int i = -7, r = -7;
    CHECK(c.index(order[n].second, order[n].first) == (long long)n);
    c.cell((long long)n, i, r);
    CHECK(i == order[n].second && r == order[n].first);
  }
  // (d) the lines: row r by ascending i, input position i by ascending r
  long long at = 0;
  for (int r = 0; r <= L; ++r) {
    CHECK(c.template lineFirst<0>(r) == at);
    for (int i = 0; i <= I; ++i)
      if (mem.count({r, i})) {
        int ci = -7, cr = -7;
        c.template lineCell<0>(at++, ci, cr);
        CHECK(ci == i && cr == r);
      }
  }
  if (columns) {
    at = 0;
    for (int i = 0; i <= I; ++i) {
      CHECK(c.template lineFirst<1>(i) == at);
      for (int r = 0; r <= L; ++r)
        if (mem.count({r, i})) {
          int ci = -7, cr = -7;
          c.template lineCell<1>(at++, ci, cr);
          CHECK(ci == i && cr == r);
        }
    }
    CHECK(at == c.cells());
  }
  // (e) the ring: no two cells of the diagonals d, d - 1, d - 2 share a slot
  for (int d = 0; d <= I + L; ++d) {
    std::set<long long> slots;
    for (int e = d; e >= 0 && e >= d - 2; --e)
      for (const auto &ri : byDiag[(size_t)e]) {
        const long long s = c.slot(ri.second, ri.first);
        CHECK(s >= 0 && s < 3LL * c.M && slots.insert(s).second);
      }
  }
}

static std::map<std::string, long long> g_tally;

// st / en through the real builder; an accepted envelope is checked with and without its transposed tables
static bool envelope(int I, int L, const std::vector<int32_t> &st, const std::vector<int32_t> &en) {
  static EnvHost h(1);
  g_I = I; g_L = L; g_st = &st; g_en = &en;
  const char *msg = env_add(h, 0, I, L, (long long)st.size(), st.data(), en.data(), false);
  if (msg) {
    CHECK(!std::strcmp(msg, "Envelope/sequence mismatch") || !std::strcmp(msg, "Envelope is not connected") || !std::strcmp(msg, "Envelope is not monotone"));
    CHECK(h.st.empty() && h.lo.empty() && h.envBase[0] == -1);      // a rejected envelope leaves nothing behind
    ++g_tally[msg];
    return false;
  }
  ++g_tally["accepted"];
  EnvHost hc(1);
  CHECK(env_add(hc, 0, I, L, (long long)st.size(), st.data(), en.data(), true) == nullptr);
  Members mem;
  for (int r = 0; r <= L; ++r)
    for (int i = st[(size_t)r]; i < en[(size_t)r]; ++i) mem.insert({r, i});
  check(h.cells(0, I, L), I, L, mem, true, true, false);
  check(hc.cells(0, I, L), I, L, mem, true, true, true);
  h = EnvHost(1);
  return true;
}

// every st / en with values in lo .. hi, row after row; ordered: only rows with st <= en
static void enumerate(int I, int L, int lo, int hi, bool ordered) {
  std::vector<std::pair<int, int>> rows;
  for (int a = lo; a <= hi; ++a)
    for (int b = ordered ? a : lo; b <= hi; ++b) rows.push_back({a, b});
  std::vector<size_t> pick((size_t)L + 1, 0);
  std::vector<int32_t> st((size_t)L + 1), en((size_t)L + 1);
  g_case = "enumerated";
  for (;;) {
    for (int r = 0; r <= L; ++r) { st[(size_t)r] = rows[pick[(size_t)r]].first; en[(size_t)r] = rows[pick[(size_t)r]].second; }
    envelope(I, L, st, en);
    int r = 0;      // the next combination, as an odometer
    while (r <= L && ++pick[(size_t)r] == rows.size()) pick[(size_t)r++] = 0;
    if (r > L) return;
  }
}

static void band(int I, int L, int halfWidth) {
  std::vector<int32_t> st((size_t)L + 1), en((size_t)L + 1);
  for (int r = 0; r <= L; ++r) {
    const int centre = L ? (int)((long long)r * I / L) : 0;
    st[(size_t)r] = std::max(0, centre - halfWidth); en[(size_t)r] = std::min(I + 1, centre + halfWidth + 1);
  }
  g_case = "band";
  CHECK(envelope(I, L, st, en));
}

int main() {
  const int rect[][2] = {{0, 0}, {0, 3}, {3, 0}, {1, 1}, {2, 5}, {5, 2}, {4, 4}};
  for (const auto &s : rect) {
    const int I = s[0], L = s[1];
    g_case = "rectangle"; g_I = I; g_L = L; g_st = g_en = nullptr;
    Members mem;
    for (int r = 0; r <= L; ++r)
      for (int i = 0; i <= I; ++i) mem.insert({r, i});
    check(RectCells(I, L), I, L, mem, false, false, true);
    // the same cells as a full envelope
    CHECK(envelope(I, L, std::vector<int32_t>((size_t)L + 1, 0), std::vector<int32_t>((size_t)L + 1, I + 1)));
  }
  // every envelope for I, L <= 4: all st <= en within 0 .. I + 1 (no other row passes the first check) ...
  for (int I = 0; I <= 4; ++I)
    for (int L = 0; L <= 4; ++L) enumerate(I, L, 0, I + 1, true);
  // ... and for I, L <= 2 every st / en in -1 .. I + 2, reversed and out-of-range rows included
  for (int I = 0; I <= 2; ++I)
    for (int L = 0; L <= 2; ++L) enumerate(I, L, -1, I + 2, false);
  CHECK(g_tally["accepted"] > 0 && g_tally["Envelope/sequence mismatch"] > 0 && g_tally["Envelope is not connected"] > 0 && g_tally["Envelope is not monotone"] > 0);
  // one rejection of each kind, by hand
  {
    g_case = "by hand"; g_st = g_en = nullptr;
    const int32_t st[] = {0, 1, 0}, en[] = {2, 3, 4}, far[] = {1, 1, 1}, wide[] = {2, 3, 5};
    EnvHost h(1);
    CHECK(!std::strcmp(env_add(h, 0, 3, 2, 3, st, en, true), "Envelope is not monotone"));
    CHECK(!std::strcmp(env_add(h, 0, 3, 2, 3, far, en, true), "Envelope is not connected"));
    CHECK(!std::strcmp(env_add(h, 0, 3, 2, 3, st, wide, true), "Envelope/sequence mismatch"));
    CHECK(!std::strcmp(env_add(h, 0, 3, 3, 3, st, en, true), "Envelope/sequence mismatch"));
  }
  band(70, 3, 15);      // i passes 64 (M stays within min(I, L) + 1)
  band(3, 70, 1);
  band(70, 70, 40);     // M passes 64
  std::printf("LATTICE OK");
  for (const auto &t : g_tally) std::printf("  %s: %lld", t.first.c_str(), t.second);
  std::printf("\n");
  return 0;
}
