#!/usr/bin/env python3
"""eval_bra_v2: held-out metrics of a brake-net checkpoint (bra_*.th) on recorded routes - precision / recall of the agent's
`pred_bra > 0.1`, AP, and the IoU of its two segmentation heads (lav_amd.train.evaluate_camera; the reference has no counterpart).
Single process.

    python eval_bra_v2.py --synthetic --frames 2
    python eval_bra_v2.py --config-path config_v2.yaml --data-dir /data/held_out --bra bra_10.th
    python eval_bra_v2.py --synthetic --frames 2 --precision all   # the same frames at f16x3, bf16x6 and f32, side by side"""
from lav_amd.train.evaluate_camera import main

if __name__ == "__main__":
    main("bra")
