// channel_plan.h — the host-only arithmetic of the entry points that return named channels into the caller's arrays (first
// hits, hit surfaces, lightmap lookups, probe volumes, path vertices, AOVs, lightmap bakes).  A call's output
// struct has ONE table, a Row per channel, written in staging order; everything that walks the channels walks it: the null
// check (first_null), the staging layout inside one f64 allocation of the handle (layout), and — api_internal.h, they need HIP
// — the caller's arrays offset to a piece, the arrays inside the allocation and the copy out.  No HIP, no handle:
// tests/cpp/channel_plan_check.cpp builds it and every table alone, with the host sanitizers too.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace rptchan {

inline uint64_t even(uint64_t w) { return (w + 1) / 2 * 2; }
inline uint64_t i32_words(uint64_t count) { return even((count + 1) / 2); } // `count` int32 values, in f64 words
inline uint64_t u8_words(uint64_t count) { return even((count + 7) / 8); }  // `count` bytes, in f64 words

// ---- a channel: its bit, `comps` components of `bytes` bytes (8, 4 or 1) per element, which of a call's two counts its
// elements follow (0: the items — rays, texels, vertices; 1: the paths, which only path vertices have), where its pointer
// stands in the caller's struct, and what the null check says.  A row the caller never sees (an array the handle keeps for
// its own kernels) has a bit outside the header's and NO_MEMBER
constexpr int MAX_ROWS = 12;
constexpr uint32_t NO_MEMBER = ~0u;
struct Row {
  uint32_t bit;
  uint8_t comps, bytes, per_path;
  uint32_t member;
  const char* null_text;
};
#define RPT_CHANNEL_ROW(Struct, BIT, member, comps, bytes, per_path) \
  rptchan::Row { BIT, comps, bytes, per_path, (uint32_t)offsetof(Struct, member), #Struct ": " #BIT " is named but " #member " is NULL" }
#define RPT_INTERNAL_ROW(bit, comps, bytes) \
  rptchan::Row { bit, comps, bytes, 0, rptchan::NO_MEMBER, nullptr }

// a table by reference: what the functions below and api_internal.h's take
struct Table {
  const Row* rows;
  int n;
  template <int N> constexpr Table(const Row (&r)[N]) : rows(r), n(N) { static_assert(N <= MAX_ROWS, "MAX_ROWS"); }
};
// a call's counts: items, and (path vertices) paths
struct Counts {
  uint64_t n[2];
  Counts(uint64_t items, uint64_t paths = 0) : n{items, paths} {}
};
inline uint64_t row_bytes(const Row& r, const Counts& c) { return c.n[r.per_path] * r.comps * r.bytes; }
inline uint64_t row_words(const Row& r, const Counts& c) { // 16-byte aligned
  const uint64_t elems = c.n[r.per_path] * r.comps;
  return r.bytes == 8 ? even(elems) : r.bytes == 4 ? i32_words(elems) : u8_words(elems);
}
// the rows of `channels` in ascending bit order — the order of the null checks and of the copies out —: f(k) per row k
template <class F> void by_bit(Table t, uint32_t channels, F&& f) {
  for (uint32_t b = 1; b; b <<= 1)
    if (channels & b)
      for (int k = 0; k < t.n; k++)
        if (t.rows[k].bit == b) f(k);
}

// ---- the arrays of the rows `has` names inside ONE f64 allocation: offsets in f64 words by row (ABSENT: not there), each
// array 16-byte aligned, in row order — which is why a table is written in staging order, the f64 arrays first
constexpr uint64_t ABSENT = ~0ull;
struct Layout {
  uint64_t off[MAX_ROWS];
  uint32_t has;
  uint64_t words;
};
inline Layout layout(Table t, uint32_t has, const Counts& c) {
  Layout l{};
  for (uint64_t& o : l.off) o = ABSENT;
  for (int k = 0; k < t.n; k++)
    if (has & t.rows[k].bit) {
      l.off[k] = l.words;
      l.words += row_words(t.rows[k], c);
      l.has |= t.rows[k].bit;
    }
  return l;
}
inline uint64_t off_or_0(const Layout& l, int k) { return l.off[k] == ABSENT ? 0 : l.off[k]; } // (a planner's named field)

// ---- the null check: the row of the lowest bit of `channels` whose member of the caller's struct `s` is NULL (nullptr: none)
inline char* member_of(const Row& r, const void* s) {
  char* p;
  memcpy(&p, (const char*)s + r.member, sizeof p);
  return p;
}
inline const Row* first_null(Table t, uint32_t channels, const void* s) {
  const Row* found = nullptr;
  by_bit(t, channels, [&](int k) {
    if (!found && t.rows[k].member != NO_MEMBER && !member_of(t.rows[k], s)) found = &t.rows[k];
  });
  return found;
}

} // namespace rptchan
