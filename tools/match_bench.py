#!/usr/bin/env python3
"""Times ufm_amd.matching.extract_matches (csrc/matches.hip) on the device, by HIP events around back-to-back calls:
  518^2, B = 8, K = 5000, cell = 8  -- the flagship batch's dense outputs (one cell reduction, one chunk per image)
  1080 x 810, B = 1, K = 5000, cell = 1 -- one full-HD frame with a candidate per pixel (54 chunks, six merge levels)
Inputs are seeded smooth flows with their inverses (most pixels valid) and random covisibilities.  Prints one line per case
and a JSON line at the end."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ufm_amd.matching import extract_matches  # noqa: E402


def inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    F = torch.stack([0.02 * xs + 3.0 + torch.sin(ys / 37.0), 0.01 * ys - 2.0 + torch.cos(xs / 29.0)]).expand(B, 2, H, W).clone()
    F += 0.05 * torch.randn(F.shape, generator=g)
    G = -F + 0.05 * torch.randn(F.shape, generator=g)  # near-inverse: cycle errors around a tenth of a pixel
    Cs, Ct = torch.rand(B, H, W, generator=g), torch.rand(B, H, W, generator=g)
    return [t.cuda() for t in (F, Cs, G, Ct)]


def time_case(B, H, W, K, cell, iters=50, warmup=5):
    F, Cs, G, Ct = inputs(B, H, W)
    for _ in range(warmup):
        out = extract_matches(F, Cs, G, Ct, num_matches=K, cell=cell)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = extract_matches(F, Cs, G, Ct, num_matches=K, cell=cell)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000.0 / iters
    return us, out.counts.cpu().tolist()


def main():
    assert torch.cuda.is_available(), "match_bench needs a GPU"
    res = {}
    for name, (B, H, W, K, cell) in {"518x518_B8_K5000_cell8": (8, 518, 518, 5000, 8), "1080x810_B1_K5000_cell1": (1, 810, 1080, 5000, 1)}.items():
        us, counts = time_case(B, H, W, K, cell)
        print(f"extract_matches {name}: {us:.1f} us per call (counts {counts})")
        res[name + "_us"] = round(us, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
