#!/usr/bin/env python3
"""eval_full_v2: open-loop metrics of a LiDAR student + planner checkpoint on recorded (held-out) routes - BEV segmentation IoU,
detection precision / recall / AP, the ego plan's and the other vehicles' forecast errors (lav_amd.train.evaluate; the reference has
no counterpart).  Single process.

    python eval_full_v2.py --synthetic --frames 8
    python eval_full_v2.py --config-path config_v2.yaml --data-dir /data/held_out --lidar lidar_64.th --uniplanner uniplanner_64.th --bev bev_160.th
    python eval_full_v2.py --synthetic --frames 8 --precision all      # the same frames at f16x3, bf16x6 and f32, side by side"""
from lav_amd.train.evaluate import main

if __name__ == "__main__":
    main()
