#!/usr/bin/env python3
"""eval_distill_v2: the LiDAR student beside the BEV teacher it was distilled from, on the same held-out frames and the same crops - per
stage (the cast and every refinement step of the plan) both networks' ADE / FDE, the student - teacher gap per mode and which of the two
was closer to the recorded future, the agreement of their command scores, and the same for the other vehicles' forecasts
(lav_amd.train.evaluate_distill; the reference has no counterpart).  The student is scored on ground-truth poses; the deployed path, with
others taken from its own detections, is what eval_full_v2.py measures.  Single process.

    python eval_distill_v2.py --synthetic --frames 8
    python eval_distill_v2.py --config-path config_v2.yaml --data-dir /data/held_out --lidar lidar_30.th --uniplanner uniplanner_30.th
    python eval_distill_v2.py --synthetic --frames 8 --bev bev_160.th        # another teacher than the uniplanner checkpoint's
    python eval_distill_v2.py --synthetic --frames 8 --precision all         # the same frames at f16x3, bf16x6 and f32, side by side"""
from lav_amd.train.evaluate_distill import main

if __name__ == "__main__":
    main()
