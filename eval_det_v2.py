#!/usr/bin/env python3
"""eval_det_v2: rotated-box metrics of a LiDAR checkpoint's box and orientation heads over recorded routes - AP by centre distance and at
IoU 0.3 / 0.5 / 0.7 of the rotated boxes, precision and recall per range from the ego, mean IoU, centre and size errors of the matched
pairs, and the heading error histogram with the share of headings that are flipped (lav_amd.train.evaluate_det; the reference has no
counterpart).  The ground-truth boxes are read from the loader's own size / orientation targets.  Needs a lidar_*.th only: the
detector runs without a planner.  The agent's size and range filters are not applied.  Single process.

    python eval_det_v2.py --synthetic --frames 8
    python eval_det_v2.py --config-path config_v2.yaml --data-dir /data/held_out --lidar lidar_7.th
    python eval_det_v2.py --config-path config_v2.yaml --data-dir /data/held_out --lidar lidar_7.th --heads both   # at-peaks beside the dense maps
    python eval_det_v2.py --synthetic --frames 8 --precision all --iou 0.5 --range-edges 10 20 40"""
from lav_amd.train.evaluate_det import main

if __name__ == "__main__":
    main()
