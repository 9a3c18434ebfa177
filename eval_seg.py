#!/usr/bin/env python3
"""eval_seg: held-out metrics of a camera segmenter checkpoint (seg_*.th) on recorded routes - the confusion matrix of the 'seg'
loader's label maps: IoU, pixel accuracy, precision / recall per class (lav_amd.train.evaluate_camera; the reference has no
counterpart).  Single process.

    python eval_seg.py --synthetic --frames 6
    python eval_seg.py --config-path config_v2.yaml --data-dir /data/held_out --seg seg_1.th
    python eval_seg.py --synthetic --frames 6 --precision all      # f16x3 and bf16x6; exact fp32: the same command under LAV_CONV_PRECISION=f32"""
from lav_amd.train.evaluate_camera import main

if __name__ == "__main__":
    main("seg")
