"""Minimal SD1.5 usage example (parity with the reference's sd_example.py).

--prediction_type v_prediction --guidance_rescale 0.7 is the setting of the
SD 2.x 768 checkpoints. --scheduler euler-a, --eta 1.0 (ddim) and
--scheduler dpm-solver --algorithm_type sde-dpmsolver++ are the stochastic
samplers: the steps' noise is seeded from the generator below."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


import argparse

import torch

from distrifuser_amd import DistriConfig, DistriSDPipeline

parser = argparse.ArgumentParser()
parser.add_argument("--prediction_type", default="epsilon", choices=["epsilon", "v_prediction"])
parser.add_argument("--guidance_rescale", type=float, default=0.0)
parser.add_argument("--scheduler", default="ddim",
                    choices=["ddim", "euler", "euler-a", "dpm-solver"])
parser.add_argument("--eta", type=float, default=None, help="ddim only, in [0, 1]")
parser.add_argument("--algorithm_type", default=None,
                    choices=["dpmsolver++", "sde-dpmsolver++"], help="dpm-solver only")
args = parser.parse_args()
sched_kw = {k: v for k, v in (("eta", args.eta), ("algorithm_type", args.algorithm_type))
            if v is not None}

distri_config = DistriConfig(height=512, width=512, mode="stale_gn")
pipeline = DistriSDPipeline.from_pretrained(
    distri_config,
    torch_dtype=torch.bfloat16 if torch.cuda.is_available() else torch.float32,
    prediction_type=args.prediction_type,
    scheduler=args.scheduler,
    **sched_kw,
)

pipeline.set_progress_bar_config(disable=distri_config.rank != 0)
image = pipeline(
    prompt="A kitten sitting in a teacup, studio lighting",
    generator=torch.Generator().manual_seed(233),
    guidance_rescale=args.guidance_rescale,
    output_type="pil",
)
if distri_config.rank == 0:
    img = image[0]
    try:
        img.save("kitten.png")
    except AttributeError:
        import numpy as np

        np.save("kitten.npy", img)
    print("saved kitten image")
