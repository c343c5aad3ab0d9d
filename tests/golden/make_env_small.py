"""Writes tests/golden/env_small.hdr (64 x 32, run-length Radiance) and env_small.npy (what assets.load_hdr returns for it: float32 [32][64][4]).
A seeded synthetic equirectangular sky: a blue-to-warm vertical gradient over a dark ground, a little noise, one 3000.0 "sun" texel and one
exact-zero texel.  python tests/golden/make_env_small.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from hybrid_rendering_amd import assets  # noqa: E402

W, H = 64, 32


def image():
    rng = np.random.RandomState(20260)
    v = ((np.arange(H) + 0.5) / H)[:, None, None]
    sky = np.array([0.25, 0.45, 1.10]) * (1.0 - v) + np.array([1.30, 0.95, 0.60]) * v
    img = np.where(v < 0.5, sky, np.array([0.12, 0.10, 0.08])) * (1.0 + 0.25 * rng.uniform(-1.0, 1.0, (H, W, 3)))
    img[:, :8] = img[:, :1]          # flat columns: runs for the run-length coder
    img[9, 41] = 3000.0              # the sun
    img[20, 5] = 0.0
    return img.astype(np.float32)


if __name__ == "__main__":
    path = os.path.join(HERE, "env_small.hdr")
    assets.save_hdr(path, image(), rle=True)
    np.save(os.path.join(HERE, "env_small.npy"), assets.load_hdr(path))
    print(path, os.path.getsize(path))
