"""`Buffer` / `Filter` (reference src/buffer.rs): the consumer of the hot path's output.
Host-side and off the timed path, exactly as in the reference; vectorised with numpy."""
import numpy as np

from .color import color_bytes


class Filter:
    """`Filter::Box(radius)` (buffer.rs:98-108); default radius 0 is a no-op."""

    def __init__(self, radius=0):
        self.radius = int(radius)

    @staticmethod
    def Box(radius):
        return Filter(radius)


class Buffer:
    """Per-pixel `Vec<Color>` as layers: samples[k] holds the k-th sample of every pixel that has one (zero elsewhere)
    and counts[p] is the length of pixel p's Vec.  A buffer filled with add_samples only has one full layer per call."""

    def __init__(self, width, height, filter=None):  # Buffer::new, buffer.rs:15-22
        self.width, self.height = int(width), int(height)
        self.filter = filter or Filter()
        self.samples = []  # one (H*W, 3) array per sample position (= per add_samples call while the counts are even)
        self.counts = np.zeros(self.width * self.height, dtype=np.int64)

    def add_sample(self, x, y, sample):  # buffer.rs:25-30
        assert 0 <= x < self.width and 0 <= y < self.height, "Invalid pixel location"
        index = int(y) * self.width + int(x)
        k = int(self.counts[index])
        if k == len(self.samples):
            self.samples.append(np.zeros((self.width * self.height, 3)))
        self.samples[k][index] = np.asarray(sample, dtype=np.float64).reshape(3)
        self.counts[index] += 1

    def add_samples(self, samples):  # buffer.rs:32-40
        s = np.asarray(samples, dtype=np.float64).reshape(-1, 3)
        assert len(s) == self.width * self.height, "Invalid sample dimension"
        if (self.counts == len(self.samples)).all():
            self.samples.append(s.copy())
        else:  # uneven lengths (add_sample): each pixel's sample goes to its own next position
            for k in np.unique(self.counts):
                idx = np.nonzero(self.counts == k)[0]
                if k == len(self.samples):
                    self.samples.append(np.zeros((self.width * self.height, 3)))
                self.samples[k][idx] = s[idx]
        self.counts += 1

    def _total(self):
        # iter().sum::<Color>() per pixel: samples added in order.  A missing sample is +0.0, which leaves a sum that
        # started at +0.0 unchanged
        total = np.zeros((self.height * self.width, 3))
        for s in self.samples:
            total = total + s
        return total

    def _filtered(self):  # get_filtered_color, buffer.rs:75-93
        assert self.samples, "Pixel found with no samples"
        w, h, r = self.width, self.height, self.filter.radius
        total = self._total().reshape(h, w, 3)
        n = self.counts.astype(np.float64).reshape(h, w, 1)
        if r == 0:
            assert (n != 0).all(), "Pixel found with no samples"
            return total / n
        acc = np.zeros((h, w, 3))
        cnt = np.zeros((h, w, 1))
        # the reference loops i (x) outer, j (y) inner: same order here so sums round alike
        for dx in range(-r, r + 1):
            for dy in range(-r, r + 1):
                ys0, ys1 = max(0, -dy), min(h, h - dy)
                xs0, xs1 = max(0, -dx), min(w, w - dx)
                acc[ys0:ys1, xs0:xs1] += total[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
                cnt[ys0:ys1, xs0:xs1] += n[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
        assert (cnt != 0).all(), "Pixel found with no samples"
        return acc / cnt

    def image(self):  # buffer.rs:43-56 -> (H, W, 3) uint8
        return color_bytes(self._filtered())

    def variance(self):  # buffer.rs:59-73
        n = self.counts.astype(np.float64)
        total = self._total()
        with np.errstate(all="ignore"):  # a pixel without samples: 0/0 = NaN, as the reference computes
            mean = total / n[:, None]
        sq = np.zeros(len(n))
        for k, s in enumerate(self.samples):
            d = s - mean
            sq = sq + np.where(self.counts > k, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], 0.0)
        with np.errstate(all="ignore"):  # one sample: 0/0 = NaN, as the reference computes
            per_pixel = sq / (n - 1.0)
        variance = 0.0
        for v in per_pixel.tolist():
            variance += v
        return variance / float(len(per_pixel))
