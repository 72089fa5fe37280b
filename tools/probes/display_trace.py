#!/usr/bin/env python3
"""For tools/trace_script.sh: one ps2 pair-and-display chain at the ps2 config (511 x 640, radius 7, range 95, SSD with
noise, NCC plain) and normalise + JET of one f32 field and of a batch of 16 at 480x640, 1080p and 4K, 20 times each, so
that `rocprofv3 --kernel-trace --stats` gives the device time of every kernel of csrc/display.hip."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from introtocomputervision_amd import display, stereo, synth  # noqa: E402

left, right, _ = synth.stereo_pair(0x5EED0F20, 511, 640)
rng = display.RNG()
noise = tuple(torch.from_numpy(display.randn((511, 640), 0, 10, rng)).cuda() for _ in range(2))
L, R = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
for _ in range(20):
    stereo.disparityPairDisplay(L, R, 7, 95, stereo.SSD, stereo.AS_WRITTEN_CUDA, 1.0, noise)
    stereo.disparityPairDisplay(L, R, 7, 95, stereo.NCC, 1)
g = torch.Generator(device="cuda").manual_seed(5)
for rows, cols in ((480, 640), (1080, 1920), (2160, 3840)):
    one = torch.randn((rows, cols), device="cuda", generator=g)
    many = torch.randn((16, rows, cols), device="cuda", generator=g)
    for _ in range(20):
        display.normalizeMinMax(one, jet=True)
        display.normalizeMinMax(many, jet=True)
torch.cuda.synchronize()
print("display_trace done")
