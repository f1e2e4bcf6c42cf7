// Host-side check of rptgpu_lookup_lightmap's sizing arithmetic (rpt_amd/csrc/lightmap_lookup_plan.h): the layout of a piece's
// arrays inside one allocation — aligned, disjoint, inside `words`, the hit's four arrays present whenever the fetch reads
// them, a host caller's channels all staged and a device caller's none —, a host caller's bindings staged back to back without
// overlap, sizes that cannot be held refused, and the launch's grid: one lane per ray.
// Usage: lightmap_lookup_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rpt_amd/csrc/lightmap_lookup_plan.h"

using namespace rptlookup;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    checks++;                                                                       \
    if (!(cond)) {                                                                  \
      failures++;                                                                   \
      std::printf("FAIL lightmap_lookup_plan_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                               \
  } while (0)

static const uint64_t Mi = 1ull << 20;

// by hand
static void sizes() {
  CHECK(launch_blocks(1) == 1 && launch_blocks(256) == 1 && launch_blocks(257) == 2 && launch_blocks(4 * Mi) == 16384);
  CHECK(needs_lookup(CH_BINDING) && needs_lookup(CH_COVERED) && needs_lookup(CH_UV) && needs_lookup(CH_VALUE) && needs_lookup(CH_ALL));
  CHECK(!needs_lookup(CH_T) && !needs_lookup(CH_OBJECT) && !needs_lookup(CH_T | CH_OBJECT) && !needs_lookup(0));
  CHECK(u8_words(0) == 0 && u8_words(1) == 2 && u8_words(16) == 2 && u8_words(17) == 4 && i32_words(1) == 2 && i32_words(5) == 4);
  // a device caller that names T and OBJECT only: no fetch, nothing of the handle's
  CHECK(layout(600, CH_T | CH_OBJECT, true).words == 0 && layout(600, CH_T | CH_OBJECT, true).has == 0);
  // ... that names everything: the walk's two outputs
  const Layout all = layout(600, CH_ALL, true);
  CHECK(all.has == (IN_PRIMITIVE | IN_BARYCENTRIC) && all.barycentric == 0 && all.primitive == 1800 && all.words == 2100);
  // ... VALUE only: the hit's four
  const Layout val = layout(600, CH_VALUE, true);
  CHECK(val.has == (CH_T | CH_OBJECT | IN_PRIMITIVE | IN_BARYCENTRIC));
  CHECK(val.t == 0 && val.barycentric == 600 && val.object == 2400 && val.primitive == 2700 && val.words == 3000);
  // a host caller, one ray: t 1 -> 2 words, barycentric 3 -> 4, uv 2, value 3 -> 4, three int32 arrays and the bytes 2 each
  const Layout odd = layout(1, CH_ALL, false);
  CHECK(odd.has == (CH_ALL | IN_PRIMITIVE | IN_BARYCENTRIC));
  CHECK(odd.t == 0 && odd.barycentric == 2 && odd.uv == 6 && odd.value == 8 && odd.object == 12 && odd.primitive == 14 &&
        odd.binding == 16 && odd.covered == 18 && odd.words == 20);
  CHECK(layout(5, CH_OBJECT, false).has == CH_OBJECT);
  // a binding of 2 triangles and a 3 x 5 map of 3 components with valid bytes, behind 10 words
  const Staged s = stage_binding(10, 2, 3, 5, 3, true);
  CHECK(s.ok && s.uvs == 10 && s.uv_words == 12 && s.map == 22 && s.map_words == 45 && s.valid == 68 && s.valid_bytes == 15 && s.end == 70);
  const Staged t = stage_binding(0, 1, 1, 1, 1, false);
  CHECK(t.ok && t.uvs == 0 && t.map == 6 && t.map_words == 1 && t.valid_bytes == 0 && t.end == 8);
  // what no allocation holds is refused, not wrapped
  CHECK(!stage_binding(0, 1, 0xffffffffu, 0xffffffffu, 3, true).ok);
  CHECK(!stage_binding(WORDS_MAX, 1, 1, 1, 1, false).ok);
  CHECK(!stage_binding(0, 1, 1, 1, 4, false).ok);
  CHECK(stage_binding(0, 0xffffffffu, 1u << 16, 1u << 16, 3, true).ok);
}

static void cover() {
  const uint64_t pieces[] = {1, 2, 3, 7, 8, 9, 255, 256, 257, 600, 65535, 4 * Mi};
  for (uint64_t piece : pieces) {
    CHECK((uint64_t)launch_blocks(piece) * BLOCK >= piece && ((uint64_t)launch_blocks(piece) - 1) * BLOCK < piece);
    for (uint32_t ch = 1; ch <= CH_ALL; ch++)
      for (int on_device = 0; on_device < 2; on_device++) {
        const Layout l = layout(piece, ch, on_device != 0);
        if (!on_device) CHECK((l.has & ch) == ch);                                       // a host caller's channels are all staged
        else CHECK(!(l.has & CH_KERNEL));                                                // a device caller's are written in place
        if (needs_lookup(ch)) {
          CHECK((l.has & IN_PRIMITIVE) && (l.has & IN_BARYCENTRIC));
          CHECK((l.has & CH_T) || (on_device && (ch & CH_T)));
          CHECK((l.has & CH_OBJECT) || (on_device && (ch & CH_OBJECT)));
        } else {
          CHECK(!(l.has & (IN_PRIMITIVE | IN_BARYCENTRIC)));
        }
        struct Span { uint64_t lo, hi; };
        std::vector<Span> spans;
        if (l.has & CH_T) spans.push_back({l.t * 8, l.t * 8 + piece * 8});
        if (l.has & IN_BARYCENTRIC) spans.push_back({l.barycentric * 8, l.barycentric * 8 + 3 * piece * 8});
        if (l.has & CH_UV) spans.push_back({l.uv * 8, l.uv * 8 + 2 * piece * 8});
        if (l.has & CH_VALUE) spans.push_back({l.value * 8, l.value * 8 + 3 * piece * 8});
        if (l.has & CH_OBJECT) spans.push_back({l.object * 8, l.object * 8 + piece * 4});
        if (l.has & IN_PRIMITIVE) spans.push_back({l.primitive * 8, l.primitive * 8 + piece * 4});
        if (l.has & CH_BINDING) spans.push_back({l.binding * 8, l.binding * 8 + piece * 4});
        if (l.has & CH_COVERED) spans.push_back({l.covered * 8, l.covered * 8 + piece});
        bool ok = true;
        for (size_t i = 0; i < spans.size(); i++) {
          ok = ok && spans[i].lo % 16 == 0 && spans[i].hi <= l.words * 8;
          for (size_t j = 0; j < i; j++) ok = ok && (spans[i].lo >= spans[j].hi || spans[j].lo >= spans[i].hi);
        }
        CHECK(ok);
        CHECK(spans.empty() == (l.words == 0));
      }
  }
  // bindings back to back: each array aligned, inside its binding's span, and the spans in order
  const uint32_t tris[] = {0, 1, 2, 12, 1001}, sizes[] = {1, 2, 3, 5, 16, 2048};
  uint64_t base = 0;
  for (uint32_t n : tris)
    for (uint32_t w : sizes)
      for (uint32_t h : sizes)
        for (uint32_t comp : {1u, 3u})
          for (int has_valid = 0; has_valid < 2; has_valid++) {
            const Staged s = stage_binding(base, n, w, h, comp, has_valid != 0);
            CHECK(s.ok && s.uvs == base && s.uvs % 2 == 0 && s.map % 2 == 0 && s.valid % 2 == 0 && s.end % 2 == 0);
            CHECK(s.uv_words == 6ull * n && s.map_words == (uint64_t)w * h * comp && s.valid_bytes == (has_valid ? (uint64_t)w * h : 0));
            CHECK(s.uvs + s.uv_words <= s.map && s.map + s.map_words <= s.valid && s.valid * 8 + s.valid_bytes <= s.end * 8);
            base = s.end;
          }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
