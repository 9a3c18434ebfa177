"""Seeded builders of small cases for the camera evaluation tests (tests/test_eval_camera_host.py, tests/test_gpu_eval_camera.py).

A map case is a dict of eval_seg's arguments as NumPy arrays (logits, labels, scale); a score case of eval_scores' (scores, flags,
threshold).  Logits are continuous random numbers (no accidental ties) with one channel per pixel lifted so that the predictions cycle
through every class; the labels cycle through every class too, at another stride, so that every cell of the confusion matrix is hit
where the map is large enough.  On top of that a few pixels are planted: ties (the lower index must win), a NaN in the first, a middle
and the last channel, +Inf and -Inf, and labels out of range (k and 255)."""
from __future__ import annotations

import numpy as np

# the cases of tests/test_gpu_eval_camera.py: (n, k, h, w, scale)
SHAPES = {
    "odd_37x53": (2, 5, 37, 53, 1),          # no multiple of 4: planes start off a 16-byte boundary, the last quad is partial
    "scale4_9x13": (1, 4, 9, 13, 4),         # labels 36 x 52
    "one_pixel": (3, 2, 1, 1, 1),            # degenerate
    "eight_classes": (1, 8, 8, 4, 2),        # the largest k
    "eight_classes_16x12": (1, 8, 16, 12, 2),   # ... on a map with room for every one of its 64 cells
    "agent_3x288x256": (3, 5, 288, 256, 1),  # the agent's call; more quads (55 296) than one pass of the grid (128 x 256)
    "wide_head": (1, 4, 72, 192, 4),         # the brake net's wide head against 288 x 768 labels
}


def seg_case(seed, n, k, h, w, scale, plant=True):
    rng = np.random.default_rng(seed)
    N = n * h * w
    logits = rng.normal(0.0, 1.0, (n, k, h, w)).astype(np.float32)
    flat = logits.transpose(0, 2, 3, 1).reshape(N, k)                    # (a copy: written back below)
    order = rng.permutation(N)
    target = np.arange(N) % k
    flat[order, target] += 6.0                                           # pixel order[i] predicts class i % k
    labels = ((np.arange(N * scale * scale) * 7 // 3) % k).astype(np.uint8)[rng.permutation(N * scale * scale)]
    labels[rng.permutation(labels.size)[:k]] = np.arange(k)              # every label occurs, whatever the size
    planted = []
    if plant:
        last = k - 1
        recipes = [("tie", (0, last)), ("nan", 0), ("inf", last), ("nan", k // 2), ("tie", (last - 1, last)), ("-inf", 0), ("nan", last), ("tie_all", None)]
        for (kind, arg), px in zip(recipes[:max(0, N - k)], order[::-1]):     # from the far end of `order`: the first k keep their classes
            if kind == "tie":
                flat[px] = -3.0
                flat[px, list(arg)] = 5.0
            elif kind == "tie_all":
                flat[px] = 0.25
            else:
                flat[px, arg] = dict(nan=np.nan, inf=np.inf)[kind] if kind != "-inf" else -np.inf
            planted.append((kind, int(px)))
        spots = rng.permutation(labels.size)[:min(4, max(0, labels.size - k))]
        labels[spots] = np.array([k, 255, k + 1, 200], np.uint8)[:len(spots)]
    logits = np.ascontiguousarray(flat.reshape(n, h, w, k).transpose(0, 3, 1, 2))
    return dict(logits=logits, labels=np.ascontiguousarray(labels.reshape(n, h * scale, w * scale)), scale=scale, planted=planted)


def shape_case(name):
    n, k, h, w, scale = SHAPES[name]
    return seg_case(1000 + sum(map(ord, name)), n, k, h, w, scale)


def score_edges(threshold):
    """float32 scores on the rules' edges: the threshold itself where it is a float32 number (not above), the two ends, just below 1,
    below 0, far outside (the product with nbins overflows), NaN, +Inf, -Inf."""
    return np.array([threshold, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), -0.5, -3e38, 3e38, np.nan, np.inf, -np.inf,
                     np.nextafter(np.float32(threshold), np.float32(1))], np.float32)


def scores_case(seed, n, threshold=0.25):
    rng = np.random.default_rng(seed)
    scores = rng.uniform(-0.05, 1.05, n).astype(np.float32)
    flags = (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)     # (a flag is any non-zero byte)
    edges = score_edges(threshold)
    if n >= 2 * len(edges):                       # every edge under both flags
        scores[:2 * len(edges)] = np.concatenate([edges, edges])
        flags[:len(edges)], flags[len(edges):2 * len(edges)] = 0, 3
    return dict(scores=scores, flags=flags, threshold=threshold)
