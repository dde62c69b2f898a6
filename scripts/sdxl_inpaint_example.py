"""Inpainting usage example, launched like sdxl_example.py:

  torchrun --nproc_per_node=2 scripts/sdxl_inpaint_example.py --image in.npy --mask mask.npy

--image takes a .npy file (uint8 [H, W, 3]) and --mask a .npy file (uint8
[H, W], 255 = repaint), or anything pillow opens when it is installed; both
must already have the pipeline's size (nothing is resized). Without --image the
script first generates an image from the prompt; without --mask it repaints
the centre square of the image. --nine-channel builds the 9-channel inpaint
U-Net (preset "sdxl-inpaint"), which --model should then point to.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


import numpy as np
import torch

from distrifuser_amd import DistriConfig, DistriSDXLPipeline


def load_array(path: str, mode: str) -> np.ndarray:
    if path.endswith(".npy"):
        arr = np.load(path)
    else:
        try:
            from PIL import Image
        except ImportError as exc:
            raise SystemExit(f"{path}: pillow is not installed; pass a .npy file") from exc
        arr = np.array(Image.open(path).convert(mode))
    return arr.astype(np.uint8)


def save_image(arr: np.ndarray, stem: str) -> str:
    try:
        from PIL import Image

        Image.fromarray(arr).save(stem + ".png")
        return stem + ".png"
    except ImportError:
        np.save(stem + ".npy", arr)
        return stem + ".npy"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image", default=None, help="input image (.npy, or a pillow format)")
    ap.add_argument("--mask", default=None, help="mask, 255 = repaint (.npy, or a pillow format)")
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--prompt", default="Astronaut in a jungle, cold color palette, muted "
                                        "colors, detailed, 8k")
    ap.add_argument("--inpaint-prompt", default="a parrot on a branch, detailed, 8k")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--size", type=int, default=1024, help="height and width of the pipeline")
    ap.add_argument("--model", default=None, help="diffusers-layout checkpoint directory")
    ap.add_argument("--nine-channel", action="store_true",
                    help="a 9-channel inpaint U-Net (preset sdxl-inpaint)")
    ap.add_argument("--out", default="astronaut_inpaint")
    args = ap.parse_args()

    distri_config = DistriConfig(height=args.size, width=args.size)
    pipeline = DistriSDXLPipeline.from_pretrained(
        distri_config,
        pretrained_model_name_or_path=args.model,
        preset="sdxl-inpaint" if args.nine_channel else "sdxl",
        torch_dtype=torch.bfloat16 if torch.cuda.is_available() else torch.float32,
    )
    pipeline.set_progress_bar_config(disable=distri_config.rank != 0)

    if args.image is not None:
        init = load_array(args.image, "RGB")
    elif args.nine_channel:
        raise SystemExit("--nine-channel cannot generate its own input: pass --image")
    else:
        # every rank generates the same image: it is the input of every rank's encode
        init = pipeline(prompt=args.prompt, num_inference_steps=args.steps,
                        generator=torch.Generator().manual_seed(233), output_type="np")[0]
    if args.mask is not None:
        mask = load_array(args.mask, "L")
    else:
        mask = np.zeros((args.size, args.size), dtype=np.uint8)
        q = args.size // 4
        mask[q : 3 * q, q : 3 * q] = 255

    result = pipeline(
        prompt=args.inpaint_prompt,
        image=init,
        mask=mask,
        strength=args.strength,
        num_inference_steps=args.steps,
        generator=torch.Generator().manual_seed(234),
        output_type="np",
    )[0]
    if distri_config.rank == 0:
        print("saved", save_image(result, args.out))


if __name__ == "__main__":
    main()
