"""The pre-traced ray stash of rpt_paths<KdFlat, false> (kernels/paths.inc, RPT_RAY_STASH=2) restated in Python over random
path histories, on top of the record ring and fold walker of tests/test_fold_ring_model.py.

A lane's stashed camera ray is traced when it is generated; a lane whose ray escaped ends that path right after the
closest hit and takes the stashed hit into the same iteration's shading, so a lane can end two paths in one iteration
(the second one only at depth 0: a stashed ray that escaped too, or a hit that does not bounce).  The model pins:

  * the ring of rpt_fold_ring_slots(B) = 3 B + 2 slots is still never overrun, and at most one record is added per
    iteration;
  * the walker never reads a header that has not been written;
  * every path is folded exactly once, deepest level first, and every sample completes once;
  * every closest-hit ray is traced (and counted) once: a path of depth D at its end took D + 1 rays;
  * no work is lost: a lane stops only with no running path, no stash and no work left."""
import random

import pytest

from test_fold_ring_model import FREE, Lane


class StashLane(Lane):
    def __init__(self, B, items):
        super().__init__(B, 0)
        self.items = items          # work left (one path per item here: the chunking does not touch the ring)
        self.stash = None           # (path id, escaped) of the pre-traced camera ray
        self.pend = False
        self.exhausted = False
        self.traced = 0             # closest-hit rays, as n_ext counts them
        self.max_recs_per_iter = 0
        self.max_ends_per_iter = 0

    def walk(self):
        """one step of the walker (paths.inc, the end of the loop body)"""
        if not self.wk:
            return
        pos = self.wrap(self.wb + self.wk)
        assert self.slot[pos] == ("rec", self.wpath, self.wk - 1), ("walker reads", pos, self.slot[pos])
        self.slot[pos] = FREE
        self.folded.append((self.wpath, self.wk - 1))
        nh = self.wrap(self.wb + self.wD + 1)
        if self.wk > 1:
            self.wk -= 1
            return
        self.finished.append(self.wpath)
        if nh != self.cb:
            assert self.slot[nh] is not FREE and self.slot[nh][0] == "hdr", ("unwritten header", nh, self.slot[nh])
            path = self.slot[nh][1]
            self.slot[nh] = FREE
            self.wD, self.wb, self.wpath, self.wk = self.meta[path], nh, path, self.meta[path]
        else:
            self.wk = 0

    def end(self):
        b = self.cb
        self.path_ended(self.path, self.depth, b)
        if self.depth:
            self.advance(b, self.depth)
        self.in_path = False

    def iteration(self, rnd, p_escape, p_end, p_refill, p_cam_escape):
        """-> False once the lane is done and its walker idle (the kernel's exit test for this lane)"""
        recs = ends = 0
        # ---- refill: this lane must, or the wave refills for others (enough empty stashes elsewhere)
        if (not self.in_path and self.stash is None and not self.exhausted) or rnd.random() < p_refill:
            if self.stash is None and not self.exhausted:
                if self.items == 0:
                    self.exhausted = True
                else:
                    self.items -= 1
                    self.stash, self.pend = (self.next_path, None), True
                    self.next_path += 1
        done = not self.in_path and self.exhausted and self.stash is None
        if done and not self.wk:
            return False
        # ---- closest hits: the pending pre-trace and the running ray, each traced once
        escaped = False
        if self.pend:
            self.traced += 1
            self.stash, self.pend = (self.stash[0], rnd.random() < p_cam_escape), False
        if self.in_path:
            self.traced += 1
            escaped = rnd.random() < p_escape
        # ---- the swap
        if self.in_path and escaped and self.stash is not None:
            self.end()
            ends += 1
        swapped = False
        if not self.in_path and self.stash is not None:
            (self.path, escaped), self.stash = self.stash, None
            self.in_path, self.depth, swapped = True, 0, True
        # ---- shading
        if self.in_path:
            if escaped or rnd.random() < p_end or self.depth >= self.B:
                assert not swapped or self.depth == 0
                self.end()
                ends += 1
            else:
                self.write(self.wrap(self.cb + 1 + self.depth), ("rec", self.path, self.depth))
                self.depth += 1
                recs += 1
        self.max_recs_per_iter = max(self.max_recs_per_iter, recs)
        self.max_ends_per_iter = max(self.max_ends_per_iter, ends)
        self.walk()
        return True


def run(B, seed, items, p_escape, p_end, p_refill, p_cam_escape):
    rnd = random.Random(seed)
    lane = StashLane(B, items)
    for _ in range(100 * items + 100):
        if not lane.iteration(rnd, p_escape, p_end, p_refill, p_cam_escape):
            break
    else:
        raise AssertionError("the lane never finished")
    assert lane.items == 0 and lane.stash is None and not lane.in_path and lane.wk == 0
    assert all(s is FREE for s in lane.slot)
    return lane


@pytest.mark.parametrize("B", [0, 1, 2, 3, 8, 16])
def test_swap_keeps_the_ring_in_bounds_and_folds_every_path_once(B):
    ends_twice = False
    for seed, (pe, pd, pr, pc) in enumerate([(0.2, 0.05, 0.3, 0.03), (0.6, 0.02, 0.05, 0.5), (0.05, 0.01, 0.9, 0.0),
                                             (0.9, 0.0, 0.0, 0.9), (0.3, 0.3, 0.5, 1.0), (0.02, 0.0, 0.2, 0.1)]):
        lane = run(B, 100 * B + seed, 3000, pe, pd, pr, pc)
        assert sorted(lane.finished) == list(range(lane.next_path))                      # every sample completes, once
        per_path = {}
        for path, level in lane.folded:
            per_path.setdefault(path, []).append(level)
        for path, levels in per_path.items():
            assert levels == list(range(lane.meta[path] - 1, -1, -1))                    # deepest first, each level once
        assert set(per_path) == {p for p, d in lane.meta.items() if d}
        ringed = [p for p in lane.finished if lane.meta[p]]
        assert ringed == sorted(ringed)                                                  # ring order
        assert lane.traced == sum(d + 1 for d in lane.meta.values())                    # one closest hit per segment
        assert lane.max_recs_per_iter <= 1 and lane.max_ends_per_iter <= 2
        ends_twice = ends_twice or lane.max_ends_per_iter == 2
    assert ends_twice or B == 0  # the histories reach the new case (with B = 0 no path outlives its first iteration)
