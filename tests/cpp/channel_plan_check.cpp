// Host-side check of the channel tables (rpt_amd/csrc/channel_plan.h and the seven tables written with it: render_plan.h
// HIT_ROWS / AOV_ROWS / VERTEX_ROWS, surface_plan.h, lightmap_lookup_plan.h, probe_volume_plan.h, lightmap_plan.h): the
// staging offsets by hand at 1 and 600 items — for hits, AOVs and vertices the figures of the formulas the drivers held before
// the tables —, every channel subset's layout — aligned, disjoint, inside `words` —, and the null check: the row, the lower bit
// of two, the text.
// Usage: channel_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rpt_amd/csrc/lightmap_lookup_plan.h"
#include "../../rpt_amd/csrc/lightmap_plan.h"
#include "../../rpt_amd/csrc/probe_volume_plan.h"
#include "../../rpt_amd/csrc/render_plan.h"
#include "../../rpt_amd/csrc/surface_plan.h"

using rptchan::Counts;
using rptchan::Layout;
using rptchan::Row;
using rptchan::Table;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    checks++;                                                                 \
    if (!(cond)) {                                                            \
      failures++;                                                             \
      std::printf("FAIL channel_plan_check.cpp:%d: %s\n", __LINE__, #cond);   \
    }                                                                         \
  } while (0)

static uint32_t all_bits(Table t) {
  uint32_t a = 0;
  for (int k = 0; k < t.n; k++) a |= t.rows[k].bit;
  return a;
}
// the layout of every row of `t`: are its offsets `want` (t.n of them) and its words `words`?
static bool lies(Table t, const Counts& c, const std::vector<uint64_t>& want, uint64_t words) {
  const Layout l = rptchan::layout(t, all_bits(t), c);
  bool ok = (int)want.size() == t.n && l.words == words && l.has == all_bits(t);
  for (int k = 0; k < t.n && ok; k++) ok = l.off[k] == want[(size_t)k];
  for (int k = t.n; k < rptchan::MAX_ROWS; k++) ok = ok && l.off[k] == rptchan::ABSENT;
  return ok;
}

// by hand
static void sizes() {
  using namespace rptchan;
  CHECK(even(0) == 0 && even(1) == 2 && even(2) == 2 && even(3) == 4);
  CHECK(i32_words(1) == 2 && i32_words(4) == 2 && i32_words(5) == 4 && i32_words(600) == 300);
  CHECK(u8_words(0) == 0 && u8_words(1) == 2 && u8_words(16) == 2 && u8_words(17) == 4 && u8_words(600) == 76);
  // first hits: t, normal, position, albedo, object
  CHECK(lies(rptplan::HIT_ROWS, 1, {0, 2, 6, 10, 14}, 16));
  CHECK(lies(rptplan::HIT_ROWS, 600, {0, 600, 2400, 4200, 6000}, 6300));
  // AOVs: depth, normal, albedo, position, hits, object; the zero fill ends behind hits
  CHECK(lies(rptplan::AOV_ROWS, 1, {0, 2, 6, 10, 14, 16}, 18));
  CHECK(lies(rptplan::AOV_ROWS, 600, {0, 600, 2400, 4200, 6000, 6300}, 6600));
  const Layout feat = layout(rptplan::AOV_ROWS, RPT_AOV_DEPTH | RPT_AOV_NORMAL | RPT_AOV_ALBEDO | RPT_AOV_POSITION | rptplan::AOV_HITS, 600);
  CHECK(feat.off[rptplan::AOV_R_HITS] == 6000 && feat.off[rptplan::AOV_R_OBJECT] == ABSENT && feat.words == 6300);
  const Layout hits_only = layout(rptplan::AOV_ROWS, rptplan::AOV_HITS, 5);
  CHECK(hits_only.off[rptplan::AOV_R_HITS] == 0 && hits_only.words == 4);
  // path vertices: length, t, normal, object, position, direction, draw, radiance, bsdf, inv_pdf, abs_cos — one ray of 3
  // samples and 3 vertices per path (9 vertices, 3 paths), 600 rays of 2 samples and 3 vertices (3600, 1200)
  CHECK(lies(rptplan::VERTEX_ROWS, rptplan::vertex_counts(1, 1, 0), {0, 2, 4, 8, 10, 14, 18, 20, 24, 28, 30}, 32));
  CHECK(lies(rptplan::VERTEX_ROWS, rptplan::vertex_counts(1, 3, 2), {0, 2, 12, 40, 46, 74, 102, 108, 136, 164, 174}, 184));
  CHECK(lies(rptplan::VERTEX_ROWS, rptplan::vertex_counts(600, 2, 2),
             {0, 600, 4200, 15000, 16800, 27600, 38400, 40200, 51000, 61800, 65400}, 69000));
  const Counts vc = rptplan::vertex_counts(600, 2, 2);
  CHECK(vc.n[0] == 3600 && vc.n[1] == 1200 && row_bytes(rptplan::VERTEX_ROWS[0], vc) == 4800 && row_bytes(rptplan::VERTEX_ROWS[2], vc) == 86400);
  // hit surfaces: t, barycentric, object, child, primitive
  CHECK(lies(rptsurface::ROWS, 1, {0, 2, 6, 8, 10}, 12));
  CHECK(lies(rptsurface::ROWS, 600, {0, 600, 2400, 2700, 3000}, 3300));
  // lightmap lookups: t, (barycentric), uv, value, object, (primitive), binding, covered
  CHECK(lies(rptlookup::ROWS, 1, {0, 2, 6, 8, 12, 14, 16, 18}, 20));
  CHECK(lies(rptlookup::ROWS, 600, {0, 600, 2400, 3600, 5400, 5700, 6000, 6300}, 6376));
  // probe volumes: t, position, normal, value, object, covered, inside
  CHECK(lies(rptvolume::ROWS, 1, {0, 2, 6, 10, 14, 16, 18}, 20));
  CHECK(lies(rptvolume::ROWS, 600, {0, 600, 2400, 4200, 6000, 6300, 6376}, 6452));
  // lightmap bakes, the whole map: irradiance, ao, barycentric, position, normal, owner
  CHECK(lies(rptlightmap::ROWS, 1, {0, 4, 6, 10, 14, 18}, 20));
  CHECK(lies(rptlightmap::ROWS, 600, {0, 1800, 2400, 4200, 6000, 7800}, 8100));
}

// every subset of a table's rows at pieces around the padding steps
static void cover_table(Table t, bool vertices) {
  const uint32_t all = all_bits(t);
  std::vector<uint32_t> bits;
  for (int k = 0; k < t.n; k++) bits.push_back(t.rows[k].bit);
  for (uint64_t piece : {1, 2, 3, 5, 7, 8, 9})
    for (uint32_t sub = 0; sub < (1u << t.n); sub++) {
      uint32_t has = 0;
      for (int k = 0; k < t.n; k++)
        if (sub >> k & 1u) has |= bits[(size_t)k];
      const Counts c = vertices ? rptplan::vertex_counts(piece, 3, 2) : Counts(piece);
      const Layout l = rptchan::layout(t, has, c);
      struct Span { uint64_t lo, hi; };
      std::vector<Span> spans;
      bool ok = l.has == has && !(has & ~all);
      for (int k = 0; k < t.n; k++) {
        const bool present = (has & t.rows[k].bit) != 0;
        ok = ok && present == (l.off[k] != rptchan::ABSENT);
        if (present) spans.push_back({l.off[k] * 8, l.off[k] * 8 + rptchan::row_bytes(t.rows[k], c)});
      }
      for (size_t i = 0; i < spans.size(); i++) {
        ok = ok && spans[i].lo % 16 == 0 && spans[i].hi > spans[i].lo && spans[i].hi <= l.words * 8;
        for (size_t j = 0; j < i; j++) ok = ok && (spans[i].lo >= spans[j].hi || spans[j].lo >= spans[i].hi);
      }
      CHECK(ok);
      CHECK(spans.empty() == (l.words == 0));
    }
}
static void cover() {
  cover_table(rptplan::HIT_ROWS, false);
  cover_table(rptplan::AOV_ROWS, false);
  cover_table(rptplan::VERTEX_ROWS, true);
  cover_table(rptsurface::ROWS, false);
  cover_table(rptlookup::ROWS, false);
  cover_table(rptvolume::ROWS, false);
  cover_table(rptlightmap::ROWS, false);
}

// ---- the null check.  `A` with every member set; then one member NULL, then two
static void set_member(void* arrays, const Row& r, char* p) { std::memcpy((char*)arrays + r.member, &p, sizeof p); }
template <class A> static void null_table(Table t, const char* const* texts) {
  static char target[8];
  A full;
  std::memset(&full, 0, sizeof full);
  int members = 0;
  for (int k = 0; k < t.n; k++)
    if (t.rows[k].member != rptchan::NO_MEMBER) {
      set_member(&full, t.rows[k], target);
      members++;
    }
  const uint32_t all = all_bits(t);
  CHECK(!rptchan::first_null(t, all, &full));
  int seen = 0;
  for (int k = 0; k < t.n; k++) {
    const Row& r = t.rows[k];
    if (r.member == rptchan::NO_MEMBER) {
      CHECK(!r.null_text);
      continue;
    }
    A one = full;
    set_member(&one, r, nullptr);
    CHECK(rptchan::first_null(t, r.bit, &one) == &r && rptchan::first_null(t, all, &one) == &r);
    CHECK(!rptchan::first_null(t, all & ~r.bit, &one)); // a channel that is not named: its pointer is not read
    bool known = false;
    for (int i = 0; i < members; i++) known = known || !std::strcmp(r.null_text, texts[i]);
    CHECK(known);
    seen++;
    for (int j = 0; j < t.n; j++) { // two NULL members: the lower bit's row
      const Row& s = t.rows[j];
      if (j == k || s.member == rptchan::NO_MEMBER) continue;
      A two = one;
      set_member(&two, s, nullptr);
      CHECK(rptchan::first_null(t, all, &two) == (r.bit < s.bit ? &r : &s));
    }
  }
  CHECK(seen == members);
  for (int i = 0; i < members; i++) { // every text belongs to exactly one row
    int rows = 0;
    for (int k = 0; k < t.n; k++) rows += t.rows[k].null_text && !std::strcmp(t.rows[k].null_text, texts[i]);
    CHECK(rows == 1);
  }
}
static void nulls() {
  static const char* const hit[] = {"RptHitArrays: RPT_HIT_T is named but t is NULL", "RptHitArrays: RPT_HIT_NORMAL is named but normal is NULL",
                                    "RptHitArrays: RPT_HIT_OBJECT is named but object is NULL",
                                    "RptHitArrays: RPT_HIT_POSITION is named but position is NULL",
                                    "RptHitArrays: RPT_HIT_ALBEDO is named but albedo is NULL"};
  null_table<RptHitArrays>(rptplan::HIT_ROWS, hit);
  static const char* const aov[] = {"RptAovBuffers: hits is NULL (it is always written)", "RptAovBuffers: RPT_AOV_DEPTH is named but depth is NULL",
                                    "RptAovBuffers: RPT_AOV_NORMAL is named but normal is NULL",
                                    "RptAovBuffers: RPT_AOV_ALBEDO is named but albedo is NULL",
                                    "RptAovBuffers: RPT_AOV_POSITION is named but position is NULL",
                                    "RptAovBuffers: RPT_AOV_OBJECT is named but object is NULL"};
  null_table<RptAovBuffers>(rptplan::AOV_ROWS, aov);
  static const char* const vertex[] = {
      "RptVertexArrays: RPT_VERTEX_LENGTH is named but length is NULL",       "RptVertexArrays: RPT_VERTEX_T is named but t is NULL",
      "RptVertexArrays: RPT_VERTEX_NORMAL is named but normal is NULL",       "RptVertexArrays: RPT_VERTEX_OBJECT is named but object is NULL",
      "RptVertexArrays: RPT_VERTEX_POSITION is named but position is NULL",   "RptVertexArrays: RPT_VERTEX_DIRECTION is named but direction is NULL",
      "RptVertexArrays: RPT_VERTEX_DRAW is named but draw is NULL",           "RptVertexArrays: RPT_VERTEX_RADIANCE is named but radiance is NULL",
      "RptVertexArrays: RPT_VERTEX_BSDF is named but bsdf is NULL",           "RptVertexArrays: RPT_VERTEX_INV_PDF is named but inv_pdf is NULL",
      "RptVertexArrays: RPT_VERTEX_ABS_COS is named but abs_cos is NULL"};
  null_table<RptVertexArrays>(rptplan::VERTEX_ROWS, vertex);
  static const char* const surface[] = {"RptSurfaceArrays: RPT_SURFACE_T is named but t is NULL",
                                        "RptSurfaceArrays: RPT_SURFACE_OBJECT is named but object is NULL",
                                        "RptSurfaceArrays: RPT_SURFACE_CHILD is named but child is NULL",
                                        "RptSurfaceArrays: RPT_SURFACE_PRIMITIVE is named but primitive is NULL",
                                        "RptSurfaceArrays: RPT_SURFACE_BARYCENTRIC is named but barycentric is NULL"};
  null_table<RptSurfaceArrays>(rptsurface::ROWS, surface);
  static const char* const lookup[] = {"RptLookupArrays: RPT_LOOKUP_T is named but t is NULL", "RptLookupArrays: RPT_LOOKUP_OBJECT is named but object is NULL",
                                       "RptLookupArrays: RPT_LOOKUP_BINDING is named but binding is NULL",
                                       "RptLookupArrays: RPT_LOOKUP_COVERED is named but covered is NULL",
                                       "RptLookupArrays: RPT_LOOKUP_UV is named but uv is NULL", "RptLookupArrays: RPT_LOOKUP_VALUE is named but value is NULL"};
  null_table<RptLookupArrays>(rptlookup::ROWS, lookup);
  static const char* const volume[] = {"RptVolumeArrays: RPT_VOLUME_T is named but t is NULL", "RptVolumeArrays: RPT_VOLUME_OBJECT is named but object is NULL",
                                       "RptVolumeArrays: RPT_VOLUME_POSITION is named but position is NULL",
                                       "RptVolumeArrays: RPT_VOLUME_NORMAL is named but normal is NULL",
                                       "RptVolumeArrays: RPT_VOLUME_VALUE is named but value is NULL",
                                       "RptVolumeArrays: RPT_VOLUME_COVERED is named but covered is NULL",
                                       "RptVolumeArrays: RPT_VOLUME_INSIDE is named but inside is NULL"};
  null_table<RptVolumeArrays>(rptvolume::ROWS, volume);
  static const char* const lightmap[] = {"RptLightmapArrays: RPT_LIGHTMAP_IRRADIANCE is named but irradiance is NULL",
                                         "RptLightmapArrays: RPT_LIGHTMAP_AO is named but ao is NULL",
                                         "RptLightmapArrays: RPT_LIGHTMAP_OWNER is named but owner is NULL",
                                         "RptLightmapArrays: RPT_LIGHTMAP_BARYCENTRIC is named but barycentric is NULL",
                                         "RptLightmapArrays: RPT_LIGHTMAP_POSITION is named but position is NULL",
                                         "RptLightmapArrays: RPT_LIGHTMAP_NORMAL is named but normal is NULL"};
  null_table<RptLightmapArrays>(rptlightmap::ROWS, lightmap);
  // the rows the caller never sees are never reported, whatever the channels say
  RptLookupArrays none;
  std::memset(&none, 0, sizeof none);
  CHECK(!rptchan::first_null(rptlookup::ROWS, rptlookup::IN_PRIMITIVE | rptlookup::IN_BARYCENTRIC, &none));
  CHECK(rptchan::first_null(rptlookup::ROWS, ~0u, &none) == &rptlookup::ROWS[rptlookup::R_T]);
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else if (!std::strcmp(s, "nulls")) nulls();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
