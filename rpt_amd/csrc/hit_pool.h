// hit_pool.h — index arithmetic of rpt_paths' wave-level pool of pre-traced camera hits (kernels/paths.inc HitPool);
// shared by the kernel and tests/cpp/hit_pool_check.cpp, free of HIP.
//
// The pool is a FIFO of `cap` slots: `head` is the slot of its oldest entry, `count` the entries it holds; both are
// wave-uniform.  The lanes of a pop mask take the oldest entries in lane order (the lane of rank r among the mask's bits
// takes entry r while r < count); the lanes of a push mask append behind the newest in lane order.  The wave only
// pushes into free slots (rpt_pool_gen_limit), so no entry is overwritten before it is popped.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPT_POOL_FN __host__ __device__ static inline
#else
#define RPT_POOL_FN static inline
#endif

// slot of the k-th entry behind the head, k < 2 cap (a pop of rank r: k = r; a push of rank r: k = count + r)
RPT_POOL_FN uint32_t rpt_pool_slot(uint32_t head, uint32_t k, uint32_t cap) { return (head + k) % cap; }
// rank of `lane` among the lanes of `mask`
RPT_POOL_FN uint32_t rpt_pool_rank(uint64_t mask, uint32_t lane) {
  return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
}
// a lane of rank r in a pop mask gets an entry
RPT_POOL_FN bool rpt_pool_pop_ok(uint32_t r, uint32_t count) { return r < count; }
// lanes that may generate in a refill: the free slots
RPT_POOL_FN uint32_t rpt_pool_gen_limit(uint32_t count, uint32_t cap) { return cap - count; }
// head and count after the lanes of `pop_mask` took what there was
RPT_POOL_FN void rpt_pool_after_pop(uint32_t& head, uint32_t& count, uint64_t pop_mask, uint32_t cap) {
  const uint32_t want = (uint32_t)__builtin_popcountll(pop_mask), n = want < count ? want : count;
  head = (head + n) % cap;
  count -= n;
}
// count after the lanes of `push_mask` appended (at most rpt_pool_gen_limit of them)
RPT_POOL_FN void rpt_pool_after_push(uint32_t& count, uint64_t push_mask) { count += (uint32_t)__builtin_popcountll(push_mask); }
// the refill predicate, at the top of an iteration in which n_need lanes will pop: at least refill_min slots are free
// (a full-width pass), or the pool cannot serve every lane that needs a hit
RPT_POOL_FN bool rpt_pool_refill(uint32_t count, uint32_t n_need, uint32_t cap, uint32_t refill_min) {
  return count + refill_min <= cap || count < n_need;
}
