"""NumPy statements of csrc/ssdhip_fit.hip: the meter's update, bit for bit, and the sum of squares -- in float64 (the truth the
kernel's float32 partials are bounded against) and in the kernel's own order of float32 additions (exact-integer data must agree with
it bit for bit)."""
import numpy as np

CHUNK = 8192                                               # SSDHIP_SUMSQ_CHUNK
LANES = 256
# The longest chain of float32 roundings an element's square passes on its way into a partial: the square itself, 31 additions in its
# lane (32 values; the first lands on an exact zero), 6 across the wave's lanes, 3 across the four waves.
DEPTH = 1 + (CHUNK // LANES - 1) + 6 + 3


def gamma(d):
    u = 2.0 ** -24
    return d * u / (1.0 - d * u)


class Meter:
    """struct ssdhip_fit_meter_state after ssdhip_fit_meter_reset, and ssdhip_fit_meter_update as `update`."""

    def __init__(self):
        self.sum, self.seen, self.steps, self.first_bad, self.last = np.float64(0.0), 0, 0, -1, np.float32(0.0)

    def update(self, loss, partials=(), l2=0.0):
        loss = np.asarray(loss, dtype=np.float32)
        b = loss.shape[0]
        s = np.float64(0.0)
        for v in loss:                                     # index order, float64
            s = s + np.float64(v)
        with np.errstate(all="ignore"):
            m = np.float32(s / np.float64(b))
            q = np.float64(0.0)
            for v in np.asarray(partials, dtype=np.float32):
                q = q + np.float64(v)
            q = np.float32(q)
            pen = np.float32(np.float32(l2) * q)           # two float32 operations, no fused multiply-add
            batch_loss = np.float32(m + pen)
            self.sum = self.sum + np.float64(batch_loss) * np.float64(b)
        self.seen += b
        self.steps += 1
        self.last = batch_loss
        if not np.isfinite(batch_loss) and self.first_bad < 0:
            self.first_bad = self.steps - 1
        return batch_loss

    @property
    def mean(self):
        return float(self.sum / self.seen)


def chunks(tensors):
    """The chunks of a table, tensor after tensor: flat arrays of at most CHUNK elements (memory order)."""
    out = []
    for t in tensors:
        t = np.asarray(t).reshape(-1)
        out += [t[i:i + CHUNK] for i in range(0, t.size, CHUNK)]
    return out


def sumsq_f64(tensors):
    """One float64 sum of squares per chunk."""
    return np.array([np.sum(np.asarray(c, dtype=np.float64) ** 2) for c in chunks(tensors)], dtype=np.float64)


def sumsq_kernel_order(tensors, vector):
    """One float32 partial per chunk in the kernel's order of additions; `vector`: values per 16-byte load (4 float32, 8 bf16)."""
    out = []
    with np.errstate(all="ignore"):
        for c in chunks(tensors):
            x = np.zeros((CHUNK,), dtype=np.float32)
            x[:c.size] = np.asarray(c, dtype=np.float32)
            x = x.reshape(CHUNK // (LANES * vector), LANES, vector).transpose(1, 0, 2).reshape(LANES, -1)   # [lane][its 32 values]
            acc = np.zeros((LANES,), dtype=np.float32)
            for k in range(x.shape[1]):
                acc = (acc + (x[:, k] * x[:, k]).astype(np.float32)).astype(np.float32)
            v = acc.reshape(LANES // 64, 64)
            s = 32
            while s >= 1:
                v = (v[:, :s] + v[:, s:2 * s]).astype(np.float32)
                s //= 2
            w = v[:, 0]
            out.append(np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3]))
    return np.array(out, dtype=np.float32)
