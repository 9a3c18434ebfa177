#!/usr/bin/env python3
"""train_bra_v2 (lav/train_bra_v2.py): the brake net RGBBrakePredictionModel([4, 10, 18]) that the agent runs every frame, one process
per GPU.

    python train_bra_v2.py --synthetic --num-epoch 1 --batch-size 52
    python train_bra_v2.py --config-path config_v2.yaml       # front and telephoto cameras of the config's data_dir ('bra' loader)

Writes <save-dir>/bra_{epoch}.th (the agent's bra_model_dir); --batch-size is the GLOBAL batch."""
from lav_amd.train.run import main

if __name__ == "__main__":
    main("bra")
