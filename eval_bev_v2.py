#!/usr/bin/env python3
"""eval_bev_v2: held-out metrics of a privileged BEV teacher checkpoint (bev_*.th) on recorded routes - ADE / FDE of the cast and of
every refinement step of the plan, per command and for braking and driving frames apart, command accuracy, and the other vehicles'
minADE, top-mode ADE / FDE and mode use (lav_amd.train.evaluate_bev; the reference has no counterpart).  Single process.

    python eval_bev_v2.py --synthetic --frames 8
    python eval_bev_v2.py --config-path config_v2.yaml --data-dir /data/held_out --bev bev_160.th
    python eval_bev_v2.py --synthetic --frames 8 --precision all   # the same frames at f16x3, bf16x6 and f32, side by side"""
from lav_amd.train.evaluate_bev import main

if __name__ == "__main__":
    main()
