#!/usr/bin/env python3
"""train_seg (lav/train_seg.py): the ERFNet camera segmenter whose probabilities the agent paints into the LiDAR points,
one process per GPU.

    python train_seg.py --synthetic --num-epoch 1 --batch-size 32
    python train_seg.py --config-path config_v2.yaml          # camera images of the config's data_dir ('seg' loader)

Writes <save-dir>/seg_{epoch}.th (RGBSegmentationModel's keys: the agent's seg_model_dir); --batch-size is the GLOBAL batch."""
from lav_amd.train.run import main

if __name__ == "__main__":
    main("seg")
