#!/usr/bin/env python3
"""eval_drive_v2: open-loop metrics of the agent's rule layer on a LiDAR student + planner checkpoint over recorded routes - precision,
recall and F1 of the LiDAR-path brake decision (plan_collide on the forecasts, pid_control's desired speed) against the expert's brake
label, what caused each brake, the same with the recorded futures in place of the forecasts, desired speed and aim point per command,
and precision / recall tables over brake_speed and the two distance limits (lav_amd.train.evaluate_drive; the reference has no
counterpart).  The camera brake net is not evaluated here (eval_bra_v2 does that).  Single process.

    python eval_drive_v2.py --synthetic --frames 8
    python eval_drive_v2.py --config-path config_v2.yaml --data-dir /data/held_out --lidar lidar_7.th --uniplanner uniplanner_7.th
    python eval_drive_v2.py --synthetic --frames 8 --agent-config team_code_v2/config.yaml --brake-speed 0.25
    python eval_drive_v2.py --synthetic --frames 8 --precision all   # the same frames at f16x3, bf16x6 and f32, side by side"""
from lav_amd.train.evaluate_drive import main

if __name__ == "__main__":
    main()
