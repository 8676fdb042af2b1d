// mb_profile_lattice.h -- the (input position i, profile row r) lattice of the pair and two-profile sweeps (mb_profile_pair.hip,
// mb_profile_pair_merge.hip, mb_profile_two.hip, mb_profile_two_merge.hip): which cells exist and where each one lives, as integers.
// RectCells is the whole rectangle, EnvCells the cells of an envelope (docs/profile_tapes.md, "Pairs under an envelope"); both answer
//
//   diag(d, ilo, nCells)    the cells of anti-diagonal d = i + r: i = ilo .. ilo + nCells - 1
//   inside(i, r)            whether the cell exists
//   index(i, r)             its number in a materialised lattice, 0 .. cells() - 1, row-major
//   slot(i, r)              its number in the rolling ring of three diagonals, 0 .. 3 M - 1
//   cells(), cell(c, i, r)  the cells of the pair and the c-th of them: the inverse of index
//   lineFirst<AXIS>(l), lineCell<AXIS>(c, i, r)
//                           the cells counted line by line, as the row posteriors do: AXIS 0, row r holds the cells
//                           lineFirst(r) .. lineFirst(r + 1) - 1 by ascending i; AXIS 1, input position i by ascending r
//
// How many doubles a cell holds and what sits beside it is the business of each family's storage adapter.  Below them env_add, which
// checks an envelope and builds the tables EnvCells reads.  Nothing here needs HIP: tests/cxx/test_lattice.cpp compiles it with g++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define MB_LATTICE_FN __host__ __device__ __forceinline__
#else
#define MB_LATTICE_FN inline
#endif

namespace mb {

struct NoTables {};      // what the rectangle needs beside a pair's descriptor

MB_LATTICE_FN int lattice_min(int a, int b) { return a < b ? a : b; }
MB_LATTICE_FN int lattice_max(int a, int b) { return a > b ? a : b; }

// The ring keeps the diagonals d, d - 1 and d - 2 that a sweep reads and writes: the M slots of diagonal d = i + r start at
// (d mod 3) * M, M at least the largest cell count of a diagonal of the pair.
MB_LATTICE_FN long long ring_diag(int i, int r, int M) { return (long long)((i + r) % 3) * M; }

// The whole rectangle of nIn + 1 input positions and nRows + 1 rows.  In the ring a cell sits at its coordinate on the short side
// of the lattice, which tells the cells of a diagonal apart.
struct RectCells {
  static constexpr bool ENV = false;
  int I, L, M, byI;
  MB_LATTICE_FN RectCells(int nIn, int nRows) : I(nIn), L(nRows), M(lattice_min(nIn, nRows) + 1), byI(nIn <= nRows) {}
  MB_LATTICE_FN void diag(int d, int &ilo, int &nCells) const { ilo = lattice_max(0, d - L); nCells = lattice_min(I, d) - ilo + 1; }
  // asked of neighbours the caller has already bounded to the rectangle
  static constexpr MB_LATTICE_FN bool inside(int, int) { return true; }
  MB_LATTICE_FN long long index(int i, int r) const { return ((long long)i * (L + 1)) + r; }
  MB_LATTICE_FN long long slot(int i, int r) const { return ring_diag(i, r, M) + (byI ? i : r); }
  MB_LATTICE_FN long long cells() const { return (long long)(I + 1) * (L + 1); }
  MB_LATTICE_FN void cell(long long c, int &i, int &r) const { i = (int)(c / (L + 1)); r = (int)(c - (long long)i * (L + 1)); }
  // (over the rectangle both line orders are a division)
  template <int AXIS> MB_LATTICE_FN long long lineFirst(int l) const { return (long long)l * ((AXIS ? L : I) + 1); }
  template <int AXIS> MB_LATTICE_FN void lineCell(long long c, int &i, int &r) const {
    const int per = (AXIS ? L : I) + 1, line = (int)(c / per), j = (int)(c - (long long)line * per);
    i = AXIS ? line : j; r = AXIS ? j : line;
  }
};

// The cells of an envelope: row r holds i = st[r] .. en[r] - 1.  Neither bound decreases from row to row, so the cells of diagonal d
// are the run i = dLo[d] .. dLo[d] + dCnt[d] - 1 (env_add builds both) and M is the largest dCnt of the pair.  In the ring a cell
// sits at i mod M: the cells of a diagonal have consecutive i and number at most M, so no two share a slot.  A slot may hold a stale
// cell of another row; it is never read, because inside() is asked first.  cSt / cOff, the transposed envelope, serve AXIS 1 alone:
// the pairs against a known input sequence pass none and never ask for it.
struct EnvCells {
  static constexpr bool ENV = true;
  const int *st, *en;         // the pair's envelope rows
  const long long *off;       // index of the first cell of each row
  const int *dLo, *dCnt;
  const int *cSt;             // the transposed envelope: first row of each input position, and
  const long long *cOff;      // the cells of the input positions before it
  long long nCells;
  int I, L, M;
  MB_LATTICE_FN EnvCells(int nIn, int nRows, const int *st, const int *en, const long long *off, const int *dLo, const int *dCnt, long long nCells, int M,
                         const int *cSt = nullptr, const long long *cOff = nullptr)
      : st(st), en(en), off(off), dLo(dLo), dCnt(dCnt), cSt(cSt), cOff(cOff), nCells(nCells), I(nIn), L(nRows), M(M) {}
  MB_LATTICE_FN void diag(int d, int &ilo, int &nCells) const { ilo = dLo[d]; nCells = dCnt[d]; }
  // r in -1..L+1, i in -1..I+1
  MB_LATTICE_FN bool inside(int i, int r) const { return r >= 0 && r <= L && i >= st[r] && i < en[r]; }
  // (r in 0..L; the index of a cell outside is formed in places, and read nowhere)
  MB_LATTICE_FN long long index(int i, int r) const { return off[r] + (i - st[r]); }
  MB_LATTICE_FN long long slot(int i, int r) const { return ring_diag(i, r, M) + (i % M); }
  MB_LATTICE_FN long long cells() const { return nCells; }
  // the last entry of o[0..n] that is <= c: the lines behind it start past the cell
  static MB_LATTICE_FN int lastLE(const long long *o, int n, long long c) {
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (o[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
  }
  MB_LATTICE_FN void cell(long long c, int &i, int &r) const { r = lastLE(off, L, c); i = st[r] + (int)(c - off[r]); }
  // (AXIS 0: the index already counts row by row, l <= L; AXIS 1: column by column through the transposed envelope, l <= I)
  template <int AXIS> MB_LATTICE_FN long long lineFirst(int l) const { return AXIS ? cOff[l] : off[l]; }
  template <int AXIS> MB_LATTICE_FN void lineCell(long long c, int &i, int &r) const {
    if (AXIS) { i = lastLE(cOff, I, c); r = cSt[i] + (int)(c - cOff[i]); }
    else cell(c, i, r);
  }
};

// The envelopes of a batch on the host, as mb_profile_pairs_set_envelopes and mb_profile_twos_set_envelopes build them: per pair
// where its rows, its diagonal runs and its columns start (-1: none), its cells and its M; the rows, their offsets, the runs and the
// columns, packed pair after pair.
struct EnvHost {
  std::vector<long long> envBase, diagBase, colBase, envCells, off, cOff;
  std::vector<int> M, st, en, lo, cnt, cSt, cEn;
  explicit EnvHost(long long n) : envBase((size_t)n, -1), diagBase((size_t)n, -1), colBase((size_t)n, -1), envCells((size_t)n, 0), M((size_t)n, 0) {}
  // what the sweeps read of pair k
  EnvCells cells(long long k, long long I, long long L) const {
    const size_t e = (size_t)envBase[(size_t)k], d = (size_t)diagBase[(size_t)k];
    const bool cols = colBase[(size_t)k] >= 0;
    return EnvCells((int)I, (int)L, st.data() + e, en.data() + e, off.data() + e, lo.data() + d, cnt.data() + d, envCells[(size_t)k], M[(size_t)k],
                    cols ? cSt.data() + colBase[(size_t)k] : nullptr, cols ? cOff.data() + colBase[(size_t)k] : nullptr);
  }
};

inline bool env_overlapping(long long s1, long long e1, long long s2, long long e2) { return !(s1 >= e2 || s2 >= e1); }

// Pair k's envelope (I input positions, L rows; `rows` entries of st / en) into h; the message of the check it fails, else null.
// Checks as mb_batch_set_envelopes (fits, connected) and that neither bound decreases from one row to the next: the sweeps rest on
// the envelope cells of an anti-diagonal being consecutive.  wantColumns: also the transposed envelope, per input position i the run
// cSt[i] .. cEn[i] - 1 of rows whose interval holds i (a run, because neither bound decreases) and cOff[i], the cells of the input
// positions before.
inline const char *env_add(EnvHost &h, long long k, long long I, long long L, long long rows, const int32_t *st, const int32_t *en, bool wantColumns) {
  if (rows != L + 1) return "Envelope/sequence mismatch";
  for (long long y = 0; y < rows; ++y)
    if (st[y] < 0 || en[y] > I + 1 || st[y] > en[y]) return "Envelope/sequence mismatch";
  bool conn = env_overlapping(st[0], en[0], 0, 1);
  for (long long y = 1; conn && y < rows; ++y) conn = env_overlapping(st[y - 1], (long long)en[y - 1] + 1, st[y], en[y]);
  conn = conn && env_overlapping(st[rows - 1], en[rows - 1], I, I + 1);
  if (!conn) return "Envelope is not connected";
  for (long long y = 1; y < rows; ++y)
    if (st[y] < st[y - 1] || en[y] < en[y - 1]) return "Envelope is not monotone";
  h.envBase[(size_t)k] = (long long)h.st.size(); h.diagBase[(size_t)k] = (long long)h.lo.size();
  const size_t d0 = h.lo.size();
  h.lo.resize(d0 + (size_t)(I + L + 1), 0); h.cnt.resize(d0 + (size_t)(I + L + 1), 0);
  long long cells = 0;
  for (long long y = 0; y < rows; ++y) {
    h.st.push_back(st[y]); h.en.push_back(en[y]); h.off.push_back(cells);
    cells += en[y] - st[y];
    // row y puts one cell on each of the diagonals st[y] + y .. en[y] - 1 + y; the rows go upwards, so on a diagonal every
    // later row holds a smaller i than the rows before it: the last one written is the diagonal's first i
    for (long long i = st[y]; i < en[y]; ++i) { h.lo[d0 + (size_t)(i + y)] = (int)i; ++h.cnt[d0 + (size_t)(i + y)]; }
  }
  h.envCells[(size_t)k] = cells;
  int M = 1;
  for (size_t d = d0; d < h.lo.size(); ++d) M = std::max(M, h.cnt[d]);
  h.M[(size_t)k] = M;
  if (wantColumns) {
    const size_t c0 = h.cSt.size();
    h.colBase[(size_t)k] = (long long)c0;
    h.cSt.resize(c0 + (size_t)I + 1, 0); h.cEn.resize(c0 + (size_t)I + 1, 0); h.cOff.resize(c0 + (size_t)I + 1, 0);
    for (long long r = L; r >= 0; --r)      // (downwards: the last row written to an input position is its first)
      for (long long i = st[r]; i < en[r]; ++i) { h.cSt[c0 + (size_t)i] = (int)r; if (!h.cEn[c0 + (size_t)i]) h.cEn[c0 + (size_t)i] = (int)r + 1; }
    long long before = 0;
    for (long long i = 0; i <= I; ++i) { h.cOff[c0 + (size_t)i] = before; before += h.cEn[c0 + (size_t)i] - h.cSt[c0 + (size_t)i]; }
  }
  return nullptr;
}

}  // namespace mb
