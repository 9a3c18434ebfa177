"""Shared by tests/test_ema_host.py and tests/test_gpu_ema.py: the distance between the specification's moving average
(lav_amd.train.optim.fused_adam_numpy(..., ema_decay=)) and a float64 recursion of the same rule, and a five-buffer twin of
tests.optim_util.World: every tensor with a shadow e at a misalignment of its own."""
import numpy as np

from lav_amd.train import optim as O
from tests.optim_util import GUARD, World, log_uniform, table_sizes

# Check b of tests/test_ema_host.py, measured on this specification (200 steps, 4 096 elements, lr 1e-2, wide_gradient's gradients): the
# worst |e - e64| / ulp(running maximum of |p|, |e|) is 2.6221 at decay 0.9 and 3.6443 at decay 0.9999.  One step's own roundings (the
# difference, the product, the sum) are worth about 1.5 ulp at that scale, and what came before is carried on multiplied by d_k: the
# longer memory of the larger decay keeps more of it, which is why 0.9999 is the worse of the two.  The bar is twice the worst
# (optim_util.BAR's convention).
MEASURED_RATIO = 3.6443
BAR = 2 * MEASURED_RATIO

# element offsets modulo 4 of (p, g, m, v, e) behind a 16-byte boundary, cycled over the tensors.  With a cycle of 6 the chunk-sized
# tensors (indices 11 .. 14: chunk - 1, chunk, chunk + 1, 2 chunk + 3) take rows 5, 0, 1 and 2 and so every path of the update kernel:
# g alone off (16-byte accesses beside 4-byte gradient loads), all equal behind a head of 3 elements (16-byte accesses), e alone off
# (4-byte accesses because of the shadow, over two chunks), all different (4-byte accesses, three chunks).  The 255 .. 257 ones take
# rows 2, 3, 4: all equal without a head and m off (4-byte accesses) at a workgroup's edge.
MISALIGN5 = [(1, 1, 1, 1, 1), (0, 0, 0, 0, 3), (0, 1, 2, 3, 1), (0, 0, 0, 0, 0), (2, 2, 1, 2, 2), (0, 3, 0, 0, 0)]
SMALL = 300         # tensors of 1 .. 7 elements behind the fifteen sizes


def ema_sizes(chunk):
    return table_sizes(chunk)[:15] + [i % 7 + 1 for i in range(SMALL)]


def float64_ema(e64, p, decay, k):
    """One step of the rule in float64 on the float32 parameters `p` of step count k, in place."""
    d = min(np.float64(decay), (1.0 + k) / (10.0 + k))
    e64 += (1.0 - d) * (p.astype(np.float64) - e64)


class EmaWorld(World):
    """tests.optim_util.World over ema_sizes with a fifth flat buffer e: rows carry `e`, offsets five entries."""

    def __init__(self, chunk, seed=0, lr=1e-2, betas=(0.9, 0.999), eps=1e-8):
        self.chunk, self.sizes = chunk, ema_sizes(chunk)
        rng = np.random.default_rng(seed)
        self.rng = rng
        cur = [0] * 5
        self.offsets = []
        for i, n in enumerate(self.sizes):
            offs = []
            for a in range(5):
                start = (cur[a] + 3) // 4 * 4 + MISALIGN5[i % len(MISALIGN5)][a]
                cur[a] = start + n
                offs.append(start)
            self.offsets.append(offs)
        self.length = max(cur) + GUARD
        self.flat = {k: np.zeros(self.length, np.float32) for k in "pgmve"}
        self.flat["p"][:] = log_uniform(rng, 1e-4, 10.0, self.length)
        self.flat["m"][:] = (rng.standard_normal(self.length) * 0.1).astype(np.float32)
        self.flat["v"][:] = np.exp(rng.uniform(np.log(1e-8), np.log(1e-1), self.length)).astype(np.float32)
        self.flat["e"][:] = log_uniform(rng, 1e-4, 10.0, self.length)        # (not p: a shadow that has a history, gaps and guards included)
        self.state = O.new_state(len(self.sizes))
        self.glob = np.zeros(1, O.GLOBAL_DTYPE)
        self.rows = []
        for i, (n, offs) in enumerate(zip(self.sizes, self.offsets)):
            row = {k: self.flat[k][o:o + n] for k, o in zip("pgmve", offs)}
            self.rows.append(dict(row, lr=lr * (1 + i % 3), beta1=betas[0], beta2=betas[1], eps=eps, state=i))
        for i in (7, 14):       # v = 0 meets g = 0 (World)
            self.rows[i]["v"][[0, self.sizes[i] - 1]] = 0.0
            self.rows[i]["m"][0] = -0.25

    def shadow_pointers(self, base, rows=None):
        """The uint64 device pointers of the shadows, row-parallel to device_table(bases, rows), for a flat e buffer at byte address `base`."""
        idx = range(len(self.rows)) if rows is None else rows
        return np.array([base + 4 * self.offsets[i][4] for i in idx], "<u8")
