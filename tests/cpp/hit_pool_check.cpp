// Host-side check of rpt_amd/csrc/hit_pool.h: the index arithmetic of rpt_paths' wave-level pool of pre-traced camera hits,
// run against a model that remembers what every slot holds.
// Usage: hit_pool_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rpt_amd/csrc/hit_pool.h"

static long long checks = 0, failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    checks++;                                                                  \
    if (!(cond)) {                                                             \
      if (failures++ < 20) std::printf("FAIL hit_pool_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                          \
  } while (0)

// the pool as the kernel keeps it, and what its slots hold: the serial number of a live entry, or -1
struct Model {
  uint32_t cap, head = 0, count = 0;
  std::vector<long long> slot;
  long long next_in = 0, next_out = 0; // serial numbers: pushed so far, popped so far
  explicit Model(uint32_t c) : cap(c), slot(c, -1) {}
  // the lanes of `mask` pop, in lane order; returns how many got an entry
  uint32_t pop(uint64_t mask) {
    uint32_t got = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
      if (!((mask >> lane) & 1ull)) continue;
      const uint32_t r = rpt_pool_rank(mask, lane);
      if (!rpt_pool_pop_ok(r, count)) continue;
      const uint32_t s = rpt_pool_slot(head, r, cap);
      CHECK(s < cap);
      CHECK(slot[s] == next_out + r); // FIFO: rank r takes the r-th oldest entry
      slot[s] = -1;
      got++;
    }
    next_out += got;
    rpt_pool_after_pop(head, count, mask, cap);
    CHECK(head < cap && count <= cap);
    return got;
  }
  // the lanes of `mask` push, in lane order (the caller keeps the mask within rpt_pool_gen_limit)
  void push(uint64_t mask) {
    for (uint32_t lane = 0; lane < 64; lane++) {
      if (!((mask >> lane) & 1ull)) continue;
      const uint32_t r = rpt_pool_rank(mask, lane);
      const uint32_t s = rpt_pool_slot(head, count + r, cap);
      CHECK(s < cap);
      CHECK(slot[s] == -1); // no entry is overwritten before it is popped
      slot[s] = next_in + r;
    }
    next_in += __builtin_popcountll(mask);
    rpt_pool_after_push(count, mask);
    CHECK(count <= cap);
  }
  uint32_t live() const {
    uint32_t n = 0;
    for (long long v : slot) n += v >= 0;
    return n;
  }
};

// masks of n bits among 64 lanes: the low lanes, the high lanes, every other lane from an odd start, a scattered one
static std::vector<uint64_t> masks_of(uint32_t n) {
  std::vector<uint64_t> out;
  if (n == 0) { out.push_back(0ull); return out; }
  const uint64_t low = n >= 64 ? ~0ull : (1ull << n) - 1ull;
  out.push_back(low);
  out.push_back(low << (64 - n));
  if (n <= 32) {
    uint64_t m = 0;
    for (uint32_t k = 0; k < n; k++) m |= 1ull << ((2 * k + 1) & 63u);
    out.push_back(m);
  }
  uint64_t m = 0;
  uint32_t lane = 5;
  for (uint32_t k = 0; k < n; k++) { // a stride of 37 lanes visits all 64
    m |= 1ull << lane;
    lane = (lane + 37u) & 63u;
  }
  out.push_back(m);
  return out;
}

// every (capacity, head, count, pop size, push size) of the small capacities, each with several lane placements: a pool
// brought to (head, count), one pop, one push into the free slots, then drained in order
static void fifo() {
  const uint32_t caps[] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  for (uint32_t cap : caps)
    for (uint32_t head = 0; head < cap; head++)
      for (uint32_t count = 0; count <= cap; count++)
        for (uint32_t np = 0; np <= cap + 2 && np <= 64; np++)
          for (uint64_t pm : masks_of(np)) {
            const uint32_t popped = np < count ? np : count;
            for (uint32_t nq = 0; nq <= cap - (count - popped); nq++)
              for (uint64_t qm : masks_of(nq)) {
                Model m(cap);
                // to (head, count): `head` entries through the pool first, then `count` that stay
                for (uint32_t k = 0; k < head; k++) { m.push(1ull); m.pop(1ull << 63); }
                CHECK(m.head == head && m.count == 0);
                for (uint32_t k = 0; k < count; k++) m.push(1ull << (k & 63u));
                CHECK(m.head == head && m.count == count && m.live() == count);
                CHECK(m.pop(pm) == popped);
                CHECK(m.count == count - popped && m.live() == m.count);
                CHECK(nq <= rpt_pool_gen_limit(m.count, cap));
                m.push(qm);
                CHECK(m.count == count - popped + nq && m.live() == m.count);
                while (m.count) m.pop(3ull << 20); // two lanes at a time: order is checked inside
                CHECK(m.next_out == m.next_in && m.live() == 0);
              }
          }
}

// a long run of the kernel's loop on a pool of the shipped shape and of small ones: random numbers of lanes that need a
// hit and of lanes with work, the refill predicate deciding
static void stream() {
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  const uint32_t shapes[][3] = {{64, 48, 64}, {64, 40, 64}, {64, 56, 64}, {64, 64, 64}, {64, 1, 64}, {96, 48, 64}, {8, 5, 8}, {5, 2, 4}, {3, 3, 3}};
  for (const auto& sh : shapes) {
    const uint32_t cap = sh[0], refill_min = sh[1], lanes = sh[2];
    Model m(cap);
    for (int it = 0; it < 20000; it++) {
      uint64_t need = rnd(), work = (it % 1000) < 900 ? rnd() | rnd() : rnd() & rnd() & rnd(); // mostly plenty of work, at times little
      if (it % 7 == 0) need |= rnd();
      if (it % 97 == 0) need = ~0ull;
      if (it % 89 == 0) work = 0ull;
      if (lanes < 64) { need &= (1ull << lanes) - 1ull; work &= (1ull << lanes) - 1ull; }
      const uint32_t n_need = (uint32_t)__builtin_popcountll(need), n_work = (uint32_t)__builtin_popcountll(work);
      uint32_t gen = 0;
      if (work != 0ull && rpt_pool_refill(m.count, n_need, cap, refill_min)) {
        const uint32_t limit = rpt_pool_gen_limit(m.count, cap);
        CHECK(limit >= 1u);
        uint64_t gm = 0;
        for (uint32_t lane = 0; lane < 64; lane++)
          if (((work >> lane) & 1ull) && rpt_pool_rank(work, lane) < limit) gm |= 1ull << lane;
        gen = (uint32_t)__builtin_popcountll(gm);
        CHECK(gen == (n_work < limit ? n_work : limit));
        m.push(gm);
      }
      // a lane that needs a hit goes without only if every lane with work has just generated
      if (work != 0ull && m.count < n_need) CHECK(gen == n_work);
      const uint32_t before = m.count;
      const uint32_t got = m.pop(need);
      CHECK(got == (n_need < before ? n_need : before));
      CHECK(m.live() == m.count);
    }
  }
}

// the refill predicate, exhaustively for the small capacities: waves of `lanes` <= cap lanes
static void refill() {
  for (uint32_t cap = 1; cap <= 16; cap++)
    for (uint32_t lanes = 1; lanes <= cap; lanes++)
      for (uint32_t refill_min = 1; refill_min <= cap; refill_min++)
        for (uint32_t count = 0; count <= cap; count++)
          for (uint32_t n_need = 0; n_need <= lanes; n_need++)
            for (uint32_t n_work = 1; n_work <= lanes; n_work++) {
              const bool r = rpt_pool_refill(count, n_need, cap, refill_min);
              const uint32_t limit = rpt_pool_gen_limit(count, cap);
              if (!r) {
                CHECK(count >= n_need);           // every lane that needs a hit finds one
                CHECK(limit < refill_min);        // and a pass would be narrower than the mark
              } else {
                CHECK(limit >= 1u);               // a refill has a slot to fill
                const uint32_t gen = n_work < limit ? n_work : limit;
                CHECK(count + gen <= cap);
                CHECK(count + gen >= n_need || gen == n_work); // short only if every cursor with work was used
              }
              CHECK(r == (limit >= refill_min || count < n_need));
            }
  // the shipped shape: a pool of 64 and a wave of 64
  for (uint32_t count = 0; count <= 64; count++)
    for (uint32_t n_need = 0; n_need <= 64; n_need++) {
      CHECK(rpt_pool_refill(count, n_need, 64, 56) == (count <= 8 || count < n_need));
      CHECK(!rpt_pool_refill(64, n_need, 64, 56));
    }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "fifo")) fifo();
  else if (!std::strcmp(s, "stream")) stream();
  else if (!std::strcmp(s, "refill")) refill();
  else { std::printf("usage: hit_pool_check fifo|stream|refill\n"); return 2; }
  if (failures) { std::printf("%lld of %lld checks failed\n", failures, checks); return 1; }
  std::printf("ok %lld\n", checks);
  return 0;
}
